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

``RendererConfig.materials = "mtl"`` shades the colour image with the OBJ's own materials (``load_obj_materials``, ``load_mtl``;
``sn_mesh_raster_color_materials`` / ``sn_mesh_cast_rays_materials``; DESIGN.md "Proxy-mesh materials"), in either lens mode.
"""

from __future__ import annotations

import ctypes as C
import math
import warnings
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
    materials: str = "none"
    """not in the reference (whose trimesh + pyrender always draw an OBJ's .mtl).  "none": the colour image is the default grey material
    or the vertex colours; ``mtllib`` / ``usemtl`` / ``vt`` are not read.  "mtl": every triangle is shaded with the material ``usemtl``
    assigned to it -- its ``Kd`` and, where there is one, its ``map_Kd`` texture (``material_defaults``; UNPINNED, DESIGN.md).  The depth
    image is the same either way"""


LENSES = ("pinhole", "camera")
MATERIAL_MODES = ("none", "mtl")


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


@dataclass
class ObjMaterial:
    """One ``newmtl`` of an .mtl file."""

    name: str
    kd: Optional[Tuple[float, float, float]] = None   # ``Kd``; None: the file gives none (``material_defaults()["missing_kd"]``)
    map_kd: Optional[str] = None                        # the resolved path of ``map_Kd``, or None
    texture: Optional[np.ndarray] = None                # [h,w,4] uint8 RGBA, rows top to bottom; None: Kd only


# number of arguments of the options of a texture statement (the .mtl specification); -o / -s / -t take one to three numbers
_MAP_OPTION_ARGS = {"-blendu": 1, "-blendv": 1, "-cc": 1, "-clamp": 1, "-texres": 1, "-bm": 1, "-boost": 1, "-imfchan": 1, "-type": 1, "-mm": 2}
_MAP_OPTION_UPTO3 = ("-o", "-s", "-t")


def _map_file_name(rest: str) -> str:
    """The file name of a ``map_Kd [options] FILE`` statement: the options are skipped (NOT applied: no scale, offset or clamp), what
    follows them is the name, spaces included."""
    while True:
        rest = rest.lstrip()
        tok = rest.split(None, 1)
        if not tok or not tok[0].startswith("-") or (tok[0] not in _MAP_OPTION_ARGS and tok[0] not in _MAP_OPTION_UPTO3):
            return rest.strip()
        rest = tok[1] if len(tok) > 1 else ""
        if tok[0] in _MAP_OPTION_ARGS:
            for _ in range(_MAP_OPTION_ARGS[tok[0]]):
                rest = (rest.split(None, 1) + [""])[1] if rest.split() else ""
        else:
            for k in range(3):
                nxt = rest.split(None, 1)
                if len(nxt) < 2:   # the last token is the file name
                    break
                try:
                    float(nxt[0])
                except ValueError:
                    break
                rest = nxt[1]


def load_mtl(path) -> List[ObjMaterial]:
    """Wavefront .mtl -> its materials in file order.  Read: ``newmtl NAME``, ``Kd r g b``, ``map_Kd [options] FILE`` (the options --
    ``-s``, ``-o``, ``-clamp``, ... -- are skipped, not applied; FILE is resolved relative to the .mtl and decoded with PIL to RGBA8).
    Every other key (``Ka Ks Ns d Tr illum map_Ks bump`` ...) is ignored.  A ``map_Kd`` file that is absent or cannot be decoded leaves
    the material Kd only, with a warning; a malformed number raises ``ValueError`` with the file and line."""
    p = Path(path)
    out: List[ObjMaterial] = []
    decoded: Dict[str, Optional[np.ndarray]] = {}
    with open(p, "r", encoding="utf8", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            key, _, rest = line.partition(" ")
            if "\t" in key:
                key, _, rest = line.partition("\t")
            rest = rest.strip()
            if key == "newmtl":
                if not rest:
                    raise ValueError(f"{p}:{ln}: newmtl needs a name")
                out.append(ObjMaterial(rest))
            elif key in ("Kd", "map_Kd"):
                if not out:
                    raise ValueError(f"{p}:{ln}: {key} before any newmtl")
                if key == "Kd":
                    parts = rest.split()
                    try:
                        kd = tuple(float(x) for x in parts[:3])
                    except ValueError as e:
                        raise ValueError(f"{p}:{ln}: bad Kd: {e}") from None
                    if len(kd) != 3 or not all(math.isfinite(x) for x in kd):
                        raise ValueError(f"{p}:{ln}: Kd needs three finite numbers")
                    out[-1].kd = kd
                else:
                    name = _map_file_name(rest)
                    if not name:
                        raise ValueError(f"{p}:{ln}: map_Kd needs a file name")
                    f = Path(name.replace("\\", "/"))
                    f = f if f.is_absolute() else p.parent / f
                    key_f = str(f)
                    if key_f not in decoded:
                        decoded[key_f] = None
                        if not f.is_file():
                            warnings.warn(f"{p}:{ln}: map_Kd file {f} not found: material {out[-1].name!r} is drawn with its Kd only")
                        else:
                            try:
                                from PIL import Image

                                with Image.open(f) as im:
                                    decoded[key_f] = np.ascontiguousarray(np.asarray(im.convert("RGBA"), dtype=np.uint8))
                            except Exception as e:   # PIL raises many types for a damaged file  # pylint: disable=broad-except
                                warnings.warn(f"{p}:{ln}: map_Kd file {f} cannot be decoded ({e}): material {out[-1].name!r} is drawn "
                                              "with its Kd only")
                    out[-1].map_kd, out[-1].texture = key_f, decoded[key_f]
    return out


def load_obj_materials(path):
    """The material side of a Wavefront OBJ, for the triangles ``load_obj`` returns (same faces, same fan, same order)
    -> (corner_uv [F,3,2] float32 or None, triangle_material [F] int32, materials: List[ObjMaterial]).

    ``vt u [v]`` and the ``b`` of ``a/b`` and ``a/b/c`` corners (1-based or negative, validated like the vertex indices) give every
    triangle its three per-CORNER texture coordinates; a face with a corner that has none gets NaN (drawn without texture), and
    corner_uv is None when no face has any.  ``usemtl NAME`` assigns the material to the faces that follow: triangle_material is its
    index in `materials`, or -1 (the default material) before any ``usemtl`` and for a name the .mtl files do not define (warned once per
    name).  ``mtllib FILE`` is resolved relative to the OBJ; an absent file gives a warning and no materials, as trimesh degrades.  An
    empty `materials` means: draw the mesh as ``materials="none"`` does."""
    p = Path(path)
    vts: List[Tuple[float, float]] = []
    uv: List[Tuple[Tuple[float, float], ...]] = []
    tri_names: List[Optional[str]] = []
    materials: List[ObjMaterial] = []
    current: Optional[str] = None
    n_verts, any_vt = 0, False
    nan2 = (math.nan, math.nan)
    with open(p, "r", encoding="utf8", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            body = line.split("#", 1)[0]
            parts = body.split()
            if not parts:
                continue
            key = parts[0]
            if key == "v":
                n_verts += 1
            elif key == "vt":
                if len(parts) < 2:
                    raise ValueError(f"{p}:{ln}: a texture coordinate needs at least u")
                try:
                    vts.append((float(parts[1]), float(parts[2]) if len(parts) > 2 else 0.0))
                except ValueError as e:
                    raise ValueError(f"{p}:{ln}: bad texture coordinate: {e}") from None
            elif key == "usemtl":
                current = body.split(None, 1)[1].strip() if len(parts) > 1 else None
            elif key == "mtllib":
                if len(parts) < 2:
                    raise ValueError(f"{p}:{ln}: mtllib needs a file name")
                whole = body.split(None, 1)[1].strip()
                names = [whole] if (p.parent / whole).is_file() or len(parts) == 2 else parts[1:]
                for name in names:
                    f = p.parent / name.replace("\\", "/")
                    if not f.is_file():
                        warnings.warn(f"{p}:{ln}: mtllib file {f} not found: its materials are not applied")
                        continue
                    have = {m.name for m in materials}
                    materials.extend(m for m in load_mtl(f) if m.name not in have)
            elif key == "f":
                corner = []
                for c in parts[1:]:
                    fields = c.split("/")
                    if len(fields) < 2 or fields[1] == "":
                        corner.append(None)
                        continue
                    try:
                        k = int(fields[1])
                    except ValueError:
                        raise ValueError(f"{p}:{ln}: bad face corner {c!r}") from None
                    if k > 0:
                        k -= 1
                    elif k < 0:
                        k += len(vts)   # relative to the texture coordinates read so far
                    else:
                        raise ValueError(f"{p}:{ln}: texture index 0 (OBJ indices start at 1)")
                    if not 0 <= k < len(vts):
                        raise ValueError(f"{p}:{ln}: texture index in {c!r} is outside the {len(vts)} texture coordinates defined so far")
                    corner.append(vts[k])
                has = all(t is not None for t in corner)
                any_vt |= has
                for i in range(1, len(corner) - 1):
                    uv.append((corner[0], corner[i], corner[i + 1]) if has else (nan2, nan2, nan2))
                    tri_names.append(current)
    index = {m.name: k for k, m in enumerate(materials)}
    unknown = sorted({n for n in tri_names if n is not None and n not in index}) if materials else []
    for n in unknown:
        warnings.warn(f"{p}: usemtl {n!r} names a material that no mtllib file defines: its faces are drawn with the default material")
    tm = np.asarray([index.get(n, -1) if n is not None else -1 for n in tri_names], dtype=np.int32)
    cuv = np.asarray(uv, dtype=np.float32).reshape(-1, 3, 2) if any_vt else None
    return cuv, tm, materials


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


def _raster(fn: str, vertices: Tensor, triangles: Tensor, mv, fx, fy, cx, cy, height, width, znear, zfar, cull_back_faces, depth,
            colors=None, shade=None) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """One call of the raster `fn` -> (color, depth).  depth: True allocates the image, a tensor is written in place, None passes NULL.
    With `shade` (the colour rasters) the colour image is allocated and `colors` -- vertex colours or None, or ``MeshMaterials`` -- goes
    with the mesh; without it color is None."""
    lib = _lib.load()
    dev = vertices.device
    opts, m = _raster_args(mv, znear, zfar, cull_back_faces)
    F = int(triangles.shape[0])
    ws_bytes = lib.sn_mesh_workspace_bytes if shade is None else lib.sn_mesh_color_workspace_bytes
    with torch.cuda.device(dev):
        color, tint, lit = None, [], []
        if shade is not None:
            held = colors.struct(dev) if isinstance(colors, MeshMaterials) else None if colors is None else colors.contiguous()
            tint, lit = [C.byref(held) if isinstance(colors, MeshMaterials) else _lib.ptr(held)], [C.byref(shade)]
            color = torch.empty((height, width, 3), dtype=torch.uint8, device=dev)
        if depth is True:
            depth = torch.empty((height, width, 1), dtype=torch.float32, device=dev)
        ws = torch.empty(max(ws_bytes(F, height, width), 1), dtype=torch.uint8, device=dev)
        _lib.check(getattr(lib, fn)(_lib.ptr(vertices), int(vertices.shape[0]), *tint, _lib.ptr(triangles), F, m, float(fx), float(fy), float(cx),
                                    float(cy), int(height), int(width), C.byref(opts), *lit, _lib.ptr(depth), *([_lib.ptr(color)] if lit else []),
                                    ws.data_ptr(), ws.numel(), _lib.current_stream()),
                   None, fn)
    return color, depth


def raster_depth(vertices: Tensor, triangles: Tensor, mv, fx: float, fy: float, cx: float, cy: float, height: int, width: int,
                 znear: float = ZNEAR, zfar: float = ZFAR, cull_back_faces: bool = True, out: Optional[Tensor] = None) -> Tensor:
    """``sn_mesh_raster_depth``: vertices [V,3] fp32 / triangles [F,3] int32 on the GPU, mv: camera-from-object [3,4] (host) ->
    z-depth [H,W,1] fp32 on the GPU, 0 where the mesh is not drawn."""
    return _raster("sn_mesh_raster_depth", vertices, triangles, mv, fx, fy, cx, cy, height, width, znear, zfar, cull_back_faces,
                   out if out is not None else True)[1]


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


TRIMESH_MISSING_KD = (0.4, 0.4, 0.4)   # trimesh's SimpleMaterial default diffuse, for a newmtl without Kd


def material_defaults() -> Dict[str, object]:
    """What stands for trimesh / pyrender when an OBJ is drawn with its .mtl (``RendererConfig.materials = "mtl"``) -- UNPINNED like
    ``shade_defaults`` (tools/make_pyrender_fixture.py --materials writes the fixtures that pin them):
      texture_srgb: the map_Kd image holds sRGB values, linearised with pow(., 2.2) (pyrender's srgb_to_linear on the base colour texture);
      default_base_color: a triangle before any usemtl, or naming a material the .mtl does not define;
      missing_kd: a newmtl without Kd;
      vertex_colors_with_materials: whether v x y z r g b colours are still applied once the file resolves a material (trimesh builds
      texture visuals then, not colour visuals)."""
    return {"texture_srgb": True, "default_base_color": PYRENDER_DEFAULT_BASE_COLOR, "missing_kd": TRIMESH_MISSING_KD,
            "vertex_colors_with_materials": False}


MATERIAL_RECORD = np.dtype([("base_color", "<f4", 4), ("texel_offset", "<u4"), ("tex_width", "<i4"), ("tex_height", "<i4"), ("reserved", "<u4")])
MAX_MATERIALS, MAX_TEXTURE_SIDE = 65535, 16384   # include/signerf_hip_mesh_material.h


class MeshMaterials:
    """The materials of a mesh as ``sn_mesh_raster_color_materials`` / ``sn_mesh_cast_rays_materials`` take them: records
    [M] ``MATERIAL_RECORD`` (``SnMeshMaterial``), triangle_material [F] int32, corner_uv [F,3,2] float32 or None, texels: the RGBA8 blob
    (uint8, 4 bytes a texel) or None.  ``on(device)`` uploads them (once per device)."""

    def __init__(self, records: np.ndarray, triangle_material: np.ndarray, corner_uv: Optional[np.ndarray] = None,
                 texels: Optional[np.ndarray] = None, texture_srgb: bool = True) -> None:
        self.records = np.ascontiguousarray(records, dtype=MATERIAL_RECORD).reshape(-1)
        self.triangle_material = np.ascontiguousarray(triangle_material, dtype=np.int32).reshape(-1)
        F = self.triangle_material.shape[0]
        self.corner_uv = None if corner_uv is None else np.ascontiguousarray(corner_uv, dtype=np.float32).reshape(F, 3, 2)
        self.texels = None if texels is None or texels.size == 0 else np.ascontiguousarray(texels, dtype=np.uint8).reshape(-1)
        self.texture_srgb = bool(texture_srgb)
        self._host = (_lib.SnMeshMaterial * max(self.records.shape[0], 1)).from_buffer_copy(
            self.records.tobytes() if self.records.shape[0] else bytes(32))
        self._on: Dict[str, Dict[str, Optional[Tensor]]] = {}

    @property
    def textured(self) -> bool:
        return self.corner_uv is not None and self.texels is not None and bool((self.records["tex_width"] > 0).any())

    def on(self, device) -> Dict[str, Optional[Tensor]]:
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = str(dev)
        if key not in self._on:
            up = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
            self._on[key] = {"records": up(self.records.view(np.uint8)), "triangle_material": up(self.triangle_material),
                             "corner_uv": up(self.corner_uv) if self.textured else None, "texels": up(self.texels)}
        return self._on[key]

    def struct(self, device) -> "_lib.SnMeshMaterials":
        """``SnMeshMaterials`` over the arrays on `device` (which this object keeps alive)."""
        t = self.on(device)
        m = _lib.SnMeshMaterials()
        m.n_materials = int(self.records.shape[0])
        m.materials = _lib.ptr(t["records"])
        m.host_materials = C.cast(self._host, C.POINTER(_lib.SnMeshMaterial))
        m.triangle_material = _lib.ptr(t["triangle_material"])
        m.corner_uv = _lib.ptr(t["corner_uv"])
        m.texels = _lib.ptr(t["texels"])
        m.texel_bytes = 0 if t["texels"] is None else int(t["texels"].numel())
        m.texture_srgb = int(self.texture_srgb)
        return m


def pack_materials(corner_uv: Optional[np.ndarray], triangle_material: np.ndarray, materials: List[ObjMaterial]) -> MeshMaterials:
    """``load_obj_materials``'s output -> ``MeshMaterials``: one record per material (``Kd`` or ``material_defaults()["missing_kd"]``,
    alpha 1), the decoded textures laid one after the other in the texel blob -- a texture that several materials name is stored once."""
    d = material_defaults()
    if not 1 <= len(materials) <= MAX_MATERIALS:
        raise ValueError(f"{len(materials)} materials: the renderer takes 1 to {MAX_MATERIALS}")
    rec = np.zeros(len(materials), dtype=MATERIAL_RECORD)
    blobs: List[np.ndarray] = []
    placed: Dict[str, Tuple[int, int, int]] = {}
    n_texels = 0
    for k, m in enumerate(materials):
        rec["base_color"][k] = list(m.kd if m.kd is not None else d["missing_kd"]) + [1.0]
        if m.texture is None:
            continue
        h, w = int(m.texture.shape[0]), int(m.texture.shape[1])
        if not (1 <= w <= MAX_TEXTURE_SIDE and 1 <= h <= MAX_TEXTURE_SIDE):
            raise ValueError(f"material {m.name!r}: its texture is {w} x {h}, the renderer takes sides of 1 to {MAX_TEXTURE_SIDE}")
        key = m.map_kd if m.map_kd is not None else f"#{k}"
        if key not in placed:
            placed[key] = (n_texels, w, h)
            blobs.append(np.ascontiguousarray(m.texture, dtype=np.uint8).reshape(-1))
            n_texels += w * h
            if n_texels >= 2 ** 32:
                raise ValueError("the textures of the mesh hold more than 2^32 texels together")
        rec["texel_offset"][k], rec["tex_width"][k], rec["tex_height"][k] = placed[key]
    texels = np.concatenate(blobs) if blobs else None
    return MeshMaterials(rec, triangle_material, corner_uv, texels, bool(d["texture_srgb"]))


def _shade_opts(base_color, ambient, background, gamma) -> "_lib.SnMeshShadeOpts":
    shade = _lib.SnMeshShadeOpts()
    shade.base_color[:] = [float(x) for x in base_color]
    shade.ambient[:] = [float(x) for x in ambient]
    shade.background[:] = [float(x) for x in background]
    shade.gamma = int(bool(gamma))
    return shade


def raster_color_materials(vertices: Tensor, triangles: Tensor, mv, fx: float, fy: float, cx: float, cy: float, height: int, width: int,
                           materials: MeshMaterials, base_color=PYRENDER_DEFAULT_BASE_COLOR, ambient=REFERENCE_AMBIENT,
                           background=PYRENDER_BACKGROUND, gamma: bool = True, znear: float = ZNEAR, zfar: float = ZFAR,
                           cull_back_faces: bool = True, with_depth: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """``sn_mesh_raster_color_materials``: ``raster_color`` with `materials` in place of the vertex colours; base_color is the default
    material (a triangle whose material index is outside the records).  The depth is bit-identical to ``raster_depth``'s."""
    F = int(triangles.shape[0])
    if int(materials.triangle_material.shape[0]) != F:
        raise ValueError(f"the materials are those of {int(materials.triangle_material.shape[0])} triangles, the mesh has {F}")
    return _raster("sn_mesh_raster_color_materials", vertices, triangles, mv, fx, fy, cx, cy, height, width, znear, zfar, cull_back_faces,
                   True if with_depth else None, materials, _shade_opts(base_color, ambient, background, gamma))


def raster_color(vertices: Tensor, triangles: Tensor, mv, fx: float, fy: float, cx: float, cy: float, height: int, width: int,
                 vertex_colors: Optional[Tensor] = None, base_color=PYRENDER_DEFAULT_BASE_COLOR, ambient=REFERENCE_AMBIENT,
                 background=PYRENDER_BACKGROUND, gamma: bool = True, znear: float = ZNEAR, zfar: float = ZFAR, cull_back_faces: bool = True,
                 with_depth: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """``sn_mesh_raster_color``: as ``raster_depth``, plus vertex_colors [V,4] uint8 RGBA on the GPU (or None) and the shading
    (``shade_defaults``) -> (color [H,W,3] uint8, depth [H,W,1] fp32 or None) on the GPU.  The depth is bit-identical to
    ``raster_depth``'s."""
    if vertex_colors is not None and (vertex_colors.dtype != torch.uint8 or tuple(vertex_colors.shape) != (int(vertices.shape[0]), 4)):
        raise ValueError(f"vertex_colors must be [V,4] uint8 with V = {int(vertices.shape[0])}, got {tuple(vertex_colors.shape)} "
                         f"{vertex_colors.dtype}")
    return _raster("sn_mesh_raster_color", vertices, triangles, mv, fx, fy, cx, cy, height, width, znear, zfar, cull_back_faces,
                   True if with_depth else None, vertex_colors, _shade_opts(base_color, ambient, background, gamma))


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


def _cast(fn: str, origins: Tensor, directions: Tensor, forward, accel: Tensor, n_triangles, height, width, znear, zfar, cull_back_faces,
          triangles, colors, n_vertices, shade) -> Tuple[Optional[Tensor], Tensor]:
    """One call of the ray cast `fn` -> (color, depth), after the checks of its arguments.  `colors`: vertex colours or None, or
    ``MeshMaterials``; with `shade` the colour image is allocated, without it color is None."""
    lib = _lib.load()
    dev = accel.device
    n = int(height) * int(width)
    if origins.numel() != 3 * n or directions.numel() != 3 * n:
        raise ValueError(f"the ray bundle holds {origins.numel() // 3} origins and {directions.numel() // 3} directions, the camera has "
                         f"{height} x {width} = {n} pixels")
    with_materials = isinstance(colors, MeshMaterials)
    if with_materials and int(colors.triangle_material.shape[0]) != int(n_triangles):
        raise ValueError(f"the materials are those of {int(colors.triangle_material.shape[0])} triangles, the mesh has {int(n_triangles)}")
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    o, d = f32(origins), f32(directions)
    if shade is not None and not with_materials and triangles is None:
        raise ValueError("with_color needs the triangles")
    if colors is not None and not with_materials and (colors.dtype != torch.uint8 or tuple(colors.shape) != (int(n_vertices), 4)):
        raise ValueError(f"vertex_colors must be [V,4] uint8 with V = {int(n_vertices)}, got {tuple(colors.shape)} {colors.dtype}")
    opts = _lib.SnMeshRaysOpts()
    opts.znear, opts.zfar, opts.cull_back_faces = float(znear), float(zfar), int(bool(cull_back_faces))
    fwd = (C.c_float * 3)(*[float(x) for x in forward])
    with torch.cuda.device(dev):
        held = colors.struct(dev) if with_materials else None if colors is None else colors.contiguous()
        depth = torch.empty((height, width, 1), dtype=torch.float32, device=dev)
        color = torch.empty((height, width, 3), dtype=torch.uint8, device=dev) if shade is not None else None
        _lib.check(getattr(lib, fn)(_lib.ptr(o), _lib.ptr(d), int(height), int(width), fwd, _lib.ptr(accel), accel.numel(), _lib.ptr(triangles),
                                    int(n_triangles), C.byref(held) if with_materials else _lib.ptr(held), int(n_vertices), C.byref(opts),
                                    C.byref(shade) if shade is not None else None, _lib.ptr(depth), _lib.ptr(color), _lib.current_stream()),
                   None, fn)
    return color, depth


def cast_rays(origins: Tensor, directions: Tensor, forward, accel: Tensor, n_triangles: int, height: int, width: int,
              triangles: Optional[Tensor] = None, vertex_colors: Optional[Tensor] = None, n_vertices: int = 0, with_color: bool = False,
              base_color=PYRENDER_DEFAULT_BASE_COLOR, ambient=REFERENCE_AMBIENT, background=PYRENDER_BACKGROUND, gamma: bool = True,
              znear: float = ZNEAR, zfar: float = ZFAR, cull_back_faces: bool = True) -> Tuple[Optional[Tensor], Tensor]:
    """``sn_mesh_cast_rays``: world-space origins / directions of height * width rays (fp32, on the GPU, row-major: what ``generate_rays``
    returns), forward: the camera's viewing axis (3 host floats), accel: ``build_accel``'s blob on the GPU -> (color [H,W,3] uint8 or None,
    z-depth [H,W,1] fp32), 0 / the background where the mesh is not drawn.  with_color needs triangles [F,3] int32 on the GPU (and takes
    vertex_colors [V,4] uint8, n_vertices = V)."""
    return _cast("sn_mesh_cast_rays", origins, directions, forward, accel, n_triangles, height, width, znear, zfar, cull_back_faces, triangles,
                 vertex_colors, n_vertices, _shade_opts(base_color, ambient, background, gamma) if with_color else None)


def cast_rays_materials(origins: Tensor, directions: Tensor, forward, accel: Tensor, n_triangles: int, height: int, width: int,
                        materials: MeshMaterials, base_color=PYRENDER_DEFAULT_BASE_COLOR, ambient=REFERENCE_AMBIENT,
                        background=PYRENDER_BACKGROUND, gamma: bool = True, znear: float = ZNEAR, zfar: float = ZFAR,
                        cull_back_faces: bool = True) -> Tuple[Tensor, Tensor]:
    """``sn_mesh_cast_rays_materials``: ``cast_rays(with_color=True)`` with `materials` in place of the vertex colours -> (color, depth);
    the depth is bit-identical to ``cast_rays``'s."""
    return _cast("sn_mesh_cast_rays_materials", origins, directions, forward, accel, n_triangles, height, width, znear, zfar, cull_back_faces,
                 None, materials, 0, _shade_opts(base_color, ambient, background, gamma))


class Renderer:
    """``Renderer`` of the reference (renderer.py:43-196): the depth it feeds the shape masking mode and the colour + depth that
    ``combine_shape_with_depth`` pastes into the aabb condition."""

    def __init__(self, config: RendererConfig, device="cuda") -> None:
        if config.lens not in LENSES:
            raise ValueError(f"RendererConfig.lens = {config.lens!r}: must be one of {', '.join(LENSES)}")
        if config.materials not in MATERIAL_MODES:
            raise ValueError(f"RendererConfig.materials = {config.materials!r}: must be one of {', '.join(MATERIAL_MODES)}")
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
        self._host_materials: Optional[MeshMaterials] = None   # materials == "mtl" and the file resolves a material

    def setup(self) -> None:
        """Parse the mesh and compute its pose (renderer.py:64-121).  Unlike the reference, a missing or non-OBJ file raises here.
        With ``lens="camera"`` the acceleration structure of the posed mesh is built here too, once.  With ``materials="mtl"`` the
        file's ``vt`` / ``usemtl`` / ``mtllib`` and the .mtl with its textures are read here (and only then); a missing .mtl or texture
        warns and degrades (``load_obj_materials``), a malformed one raises."""
        self._host_mesh = load_obj(self.object_path)
        self.pose = object_pose(self.config)
        self._host_colors, self._uploaded, self._uploaded_colors = None, {}, {}
        self._host_accel, self._uploaded_accel = None, {}
        self._host_materials = None
        if self.config.materials == "mtl":
            cuv, tm, mats = load_obj_materials(self.object_path)
            if mats:
                if int(tm.shape[0]) != int(self._host_mesh[1].shape[0]):
                    raise ValueError(f"{self.object_path}: the material reader found {int(tm.shape[0])} triangles, the mesh has "
                                     f"{int(self._host_mesh[1].shape[0])}")
                self._host_materials = pack_materials(cuv, tm, mats)
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

    def materials_on(self, device) -> Optional[MeshMaterials]:
        """The mesh's materials with their arrays on `device` (uploaded the first time a colour view of that device is rendered), or None:
        ``materials`` was "none" at ``setup()``, or the file resolves no material -- the colour image is the ``"none"`` one then."""
        verts, _ = self.mesh_on(device)
        if self._host_materials is not None:
            self._host_materials.on(verts.device)
        return self._host_materials

    def accel_on(self, device) -> Tensor:
        """``build_accel``'s blob on `device` (``lens="camera"``), uploaded the first time a view of that device is rendered."""
        verts, _ = self.mesh_on(device)
        if self._host_accel is None:
            raise RuntimeError('Renderer.setup() built no acceleration structure: RendererConfig.lens was not "camera" then')
        key = str(verts.device)
        if key not in self._uploaded_accel:
            self._uploaded_accel[key] = torch.from_numpy(self._host_accel).to(verts.device)
        return self._uploaded_accel[key]

    @staticmethod
    def _material_shade() -> Dict[str, object]:
        """``shade_defaults`` of a mesh drawn with its materials: no vertex colours, the default material for a triangle without one."""
        return dict(shade_defaults(False), base_color=material_defaults()["default_base_color"])

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
            forward = (-host[2], -host[6], -host[10])   # a nerfstudio camera looks down its -z axis
            mats = self.materials_on(dev) if with_color else None
            if mats is not None:
                return cast_rays_materials(ray_bundle.origins, ray_bundle.directions, forward, accel, int(tris.shape[0]), H, W, mats, znear=ZNEAR,
                                           zfar=ZFAR, cull_back_faces=self.config.cull_back_faces, **self._material_shade())
            vc = self.colors_on(dev) if with_color else None
            return cast_rays(ray_bundle.origins, ray_bundle.directions, forward, accel, int(tris.shape[0]), H, W, tris, vc, int(verts.shape[0]),
                             with_color, znear=ZNEAR, zfar=ZFAR, cull_back_faces=self.config.cull_back_faces, **shade_defaults(vc is not None))
        mv = model_view(host[:12], self.pose)
        if not with_color:
            return None, raster_depth(verts, tris, mv, fx, fy, cx, cy, H, W, ZNEAR, ZFAR, self.config.cull_back_faces)
        mats = self.materials_on(dev)
        if mats is not None:
            return raster_color_materials(verts, tris, mv, fx, fy, cx, cy, H, W, mats, znear=ZNEAR, zfar=ZFAR,
                                          cull_back_faces=self.config.cull_back_faces, **self._material_shade())
        vc = self.colors_on(dev)
        return raster_color(verts, tris, mv, fx, fy, cx, cy, H, W, vc, znear=ZNEAR, zfar=ZFAR, cull_back_faces=self.config.cull_back_faces,
                            **shade_defaults(vc is not None))
