"""Test-only reference of the proxy mesh drawn with its materials (``RendererConfig.materials = "mtl"``; nothing under signerf_amd/ imports
this module).  float64, built on what is there: ``raster_front`` of tests/mesh_color_oracle.py (winning triangle, barycentrics, depth
gap) and the hit finder of tests/mesh_rays_oracle.py (with its per-ray edge distance), plus

* ``sample``: the bilinear REPEAT sampler -- texel centres at (i + 0.5) / size, sampled at (u, 1 - v) (the image's top row is v = 1), the
  blend across the wrap seam takes the last and the first texel;
* ``shade``: x = ambient * Kd * tex (tex = pow(texel blend, 2.2) when texture_srgb; 1 without texture, without uv, or for a non-finite
  uv), optional pow(x, 1 / 2.2); a material index outside the list is the default material.  Like ``mesh_color_oracle.shade`` it returns
  255 * x BEFORE the rounding, and in addition per pixel ``spread``: the largest difference, in levels of 255 of the final image (after
  the sRGB round trip), among the four texels blended there -- the local slope of the picture per texel, which scales the tie window
  of the GPU tests.

It also holds the scenes of tests/test_gpu_mesh_material.py (textures, uv, material assignment), so that tests/test_mesh_material_host.py
can check their flagged shares on the CPU.
"""
from __future__ import annotations

import numpy as np

import mesh_color_oracle as mco
import mesh_oracle as mo
import mesh_rays_oracle as mro

DEFAULT_BASE = (0.3, 0.3, 0.3)


def sample(texture, u, v):
    """texture [h,w,C] (any real dtype), u, v [...] -> (blend [...,C] float64, the four texels [...,4,C] float64).  Non-finite uv: NaN."""
    tex = np.asarray(texture, dtype=np.float64)
    h, w = tex.shape[:2]
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    ok = np.isfinite(u) & np.isfinite(v)
    uu, vv = np.where(ok, u, 0.0), np.where(ok, 1.0 - v, 0.0)
    x = (uu - np.floor(uu)) * w - 0.5
    y = (vv - np.floor(vv)) * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = (x - x0)[..., None], (y - y0)[..., None]
    x0, y0 = x0.astype(np.int64) % w, y0.astype(np.int64) % h
    x1, y1 = (x0 + 1) % w, (y0 + 1) % h
    t00, t10, t01, t11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    top, bot = t00 + ax * (t10 - t00), t01 + ax * (t11 - t01)
    out = top + ay * (bot - top)
    four = np.stack([t00, t10, t01, t11], -2)
    bad = ~ok
    out[bad] = np.nan
    four[bad] = np.nan
    return out, four


def _final(tex01, kd, ambient, gamma, srgb):
    """texture value in [0, 1] (before the linearisation) -> 255 * x before the rounding"""
    t = np.power(np.maximum(tex01, 0.0), 2.2) if srgb else tex01
    x = np.asarray(ambient, dtype=np.float64) * np.asarray(kd, dtype=np.float64) * t
    if gamma:
        x = np.power(np.maximum(x, 0.0), 1.0 / 2.2)
    return 255.0 * np.clip(x, 0.0, 1.0)


def shade(tri, bary, corner_uv, triangle_material, materials, default_base=DEFAULT_BASE, ambient=(1.0, 1.0, 1.0),
          background=(1.0, 1.0, 1.0), gamma=True, texture_srgb=True):
    """tri [H,W] (-1: none), bary [H,W,3]; corner_uv [F,3,2] or None; triangle_material [F]; materials: a list of (kd (3 floats),
    texture [h,w,>=3] uint8 or None) -> (255 * x [H,W,3] float64 before the rounding, spread [H,W])."""
    H, W = tri.shape
    cov = tri >= 0
    t = np.where(cov, tri, 0)
    out = np.empty((H, W, 3))
    out[:] = 255.0 * np.clip(np.asarray(background, dtype=np.float64), 0.0, 1.0)
    spread = np.zeros((H, W))
    tm = np.asarray(triangle_material, dtype=np.int64)[t]
    known = (tm >= 0) & (tm < len(materials))
    sel = cov & ~known
    out[sel] = _final(np.ones(3), default_base, ambient, gamma, False)
    if corner_uv is not None:
        uv = (np.asarray(bary, dtype=np.float64)[..., :, None] * np.asarray(corner_uv, dtype=np.float64)[t]).sum(-2)   # [H,W,2]
    for k, (kd, texture) in enumerate(materials):
        sel = cov & known & (tm == k)
        if not sel.any():
            continue
        plain = _final(np.ones(3), kd, ambient, gamma, False)
        if texture is None or corner_uv is None:
            out[sel] = plain
            continue
        val, four = sample(np.asarray(texture)[..., :3], uv[sel][:, 0], uv[sel][:, 1])
        nouv = np.isnan(val).any(-1)
        res = _final(val / 255.0, kd, ambient, gamma, texture_srgb)
        f4 = _final(four / 255.0, np.asarray(kd, dtype=np.float64)[None, :], ambient, gamma, texture_srgb)   # [n,4,3]
        sp = (f4.max(-2) - f4.min(-2)).max(-1)
        res[nouv] = plain
        sp[nouv] = 0.0
        out[sel] = res
        spread[sel] = sp
    return out, spread


def hit_barycentrics(origins, directions, world, triangles, tri):
    """Moeller-Trumbore weights (1 - u - v, u, v) of the hits the oracle found: rays [n,3] (fp32 values), tri [n] (-1: none) -> [n,3]."""
    O = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    D = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    V = np.asarray(world, dtype=np.float64)
    T = np.asarray(triangles, dtype=np.int64)[np.where(tri >= 0, tri, 0)]
    A, B, Cc = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    e1, e2, tv = B - A, Cc - A, O - A
    pv = np.cross(D, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (e1 * pv).sum(-1)
        u = (tv * pv).sum(-1) * inv
        v = (D * np.cross(tv, e1)).sum(-1) * inv
    b = np.stack([1.0 - u - v, u, v], -1)
    b[tri < 0] = 0.0
    return b


def tie_window(spread, side):
    """The distance from a rounding boundary within which a difference of one level is a tie: 1e-3 (the window of the vertex-colour test
    for fp32-vs-float64 interpolation) + spread * S * 2^-20 (the texel-coordinate error of fp32 barycentrics -- a few 2^-23 of S texels,
    rounded up by 8 -- times the steepest local slope), S the larger texture side."""
    return 1e-3 + np.asarray(spread) * float(side) * 2.0 ** -20


def compare(got, x, spread, ok, side):
    """got [...,3] integers, x [...,3] the oracle before the rounding, ok [...]: the pixels compared -> (bad [...,3] bool, max difference)."""
    want = np.floor(x + 0.5).astype(np.int64)
    diff = np.abs(np.asarray(got).astype(np.int64) - want)
    tie = np.abs(x - np.floor(x) - 0.5) < tie_window(spread, side)[..., None]
    bad = ok[..., None] & ((diff > 1) | ((diff == 1) & ~tie))
    return bad, int(diff[ok].max()) if ok.any() else 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the scenes of tests/test_gpu_mesh_material.py
# ---------------------------------------------------------------------------------------------------------------------------------
TEXTURE_SIZES = ((64, 64), (96, 40))   # (width, height): one square power of two, one neither
MAX_SIDE = 96
KD_TEXTURED = ((0.9, 0.8, 1.0), (1.0, 1.0, 1.0))
KD_ONLY = (0.55, 0.35, 0.75)
# the three materials of the Kd-only scene: no channel's 255 * Kd^(1 / 2.2) lies within 1e-3 of a rounding boundary (asserted by
# tests/test_mesh_material_host.py), so fp32 powf cannot land on the other side
KD_EXACT = ((0.8, 0.1, 0.05), (0.2, 0.6, 0.9), (0.95, 0.45, 0.3))


def procedural_texture(width, height, seed=0, lo=0.2):
    """[height,width,4] uint8 RGBA, smooth and periodic in both axes, every colour channel in [255 * lo, 255] (the floor keeps
    pow(., 1 / 2.2) away from its infinite slope at 0, as position_colors(lo=0.2) does)."""
    x, y = np.meshgrid((np.arange(width) + 0.5) / width, (np.arange(height) + 0.5) / height)
    out = np.full((height, width, 4), 255, dtype=np.uint8)
    for c in range(3):
        kx, ky, ph = 1 + (c + seed) % 2, 1 + (c + seed + 1) % 2, 0.9 * c + 1.7 * seed
        a = 0.5 + 0.5 * np.sin(2.0 * np.pi * (kx * x + ky * y) + ph) * np.cos(2.0 * np.pi * ((2 - c % 2) * y) + 0.4 * c)
        out[..., c] = np.round(255.0 * (lo + (1.0 - lo) * a)).astype(np.uint8)
    return out


def spherical_corner_uv(vertices, triangles):
    """[F,3,2] float32: u = longitude / 2 pi + 0.5, v = 1 - colatitude / pi of each corner's direction from the mesh's centroid; the
    corners of a triangle that crosses the seam are moved to the same side of it (u up to 1.5: the REPEAT wrap is exercised)."""
    v = np.asarray(vertices, dtype=np.float64)
    p = v - v.mean(0)
    r = np.maximum(np.linalg.norm(p, axis=1), 1e-12)
    u = np.arctan2(p[:, 1], p[:, 0]) / (2.0 * np.pi) + 0.5
    w = 1.0 - np.arccos(np.clip(p[:, 2] / r, -1.0, 1.0)) / np.pi
    T = np.asarray(triangles, dtype=np.int64)
    cu, cw = u[T], w[T]
    cu = np.where((cu.max(1, keepdims=True) - cu) > 0.5, cu + 1.0, cu)
    return np.stack([cu, cw], -1).astype(np.float32)


def thirds(n_triangles):
    """material index per triangle: the first, second and last third of the mesh"""
    return np.minimum(np.arange(n_triangles) * 3 // max(n_triangles, 1), 2).astype(np.int32)


def write_scene(directory, name, vertices, triangles, corner_uv, triangle_material, materials, vertex_colors=None):
    """Writes name.obj, name.mtl and the materials' textures (PNG) into `directory` -> the OBJ's path.  materials: a list of
    (material name, kd or None, texture file name or None, texture [h,w,4] uint8 or None)."""
    import os

    from PIL import Image

    with open(os.path.join(directory, f"{name}.mtl"), "w") as fh:
        for mname, kd, tfile, tex in materials:
            fh.write(f"newmtl {mname}\nNs 250.0\nKa 1.0 1.0 1.0\n")
            if kd is not None:
                fh.write("Kd " + " ".join(f"{x:.9g}" for x in kd) + "\n")
            fh.write("Ks 0.5 0.5 0.5\nillum 2\n")
            if tfile is not None:
                fh.write(f"map_Kd {tfile}\n")
                if tex is not None and not os.path.exists(os.path.join(directory, tfile)):
                    Image.fromarray(tex, "RGBA").save(os.path.join(directory, tfile))
            fh.write("\n")
    path = os.path.join(directory, f"{name}.obj")
    with open(path, "w") as fh:
        fh.write(f"# test scene\nmtllib {name}.mtl\n")
        if vertex_colors is None:
            fh.write("".join(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in np.asarray(vertices).tolist()))
        else:
            fh.write("".join(f"v {x:.9g} {y:.9g} {z:.9g} {r / 255:.9g} {g / 255:.9g} {b / 255:.9g}\n"
                             for (x, y, z), (r, g, b, _) in zip(np.asarray(vertices).tolist(), np.asarray(vertex_colors).tolist())))
        if corner_uv is not None:
            fh.write("".join(f"vt {u:.9g} {w:.9g}\n" for u, w in np.asarray(corner_uv, dtype=np.float32).reshape(-1, 2).tolist()))
        last = None
        for k, (a, b, c) in enumerate(np.asarray(triangles).tolist()):
            m = int(triangle_material[k])
            if m != last:
                fh.write(f"usemtl {materials[m][0]}\n")
                last = m
            if corner_uv is None:
                fh.write(f"f {a + 1} {b + 1} {c + 1}\n")
            else:
                fh.write(f"f {a + 1}/{3 * k + 1} {b + 1}/{3 * k + 2} {c + 1}/{3 * k + 3}\n")
    return path


def textured_materials():
    """The three materials of the textured scenes: two textured (64 x 64 and 96 x 40, with a Kd), one Kd only
    -> (for write_scene, for shade)."""
    texs = [procedural_texture(w, h, seed=k) for k, (w, h) in enumerate(TEXTURE_SIZES)]
    files = [("square", KD_TEXTURED[0], "tex 64.png", texs[0]), ("oblong", KD_TEXTURED[1], "tex_96x40.png", texs[1]),
             ("plain", KD_ONLY, None, None)]
    return files, [(KD_TEXTURED[0], texs[0]), (KD_TEXTURED[1], texs[1]), (KD_ONLY, None)]


# the raster scenes: CASES of tests/test_gpu_mesh_color.py (the same meshes, matrices and intrinsics, so the same ambiguity flags)
def _mv(t=(0.0, 0.0, 0.0)):
    return np.hstack([np.eye(3), np.asarray(t, dtype=np.float64).reshape(3, 1)])


RASTER_CASES = {
    "icosphere": (lambda: mo.icosphere(3), _mv((0.1, -0.05, -3.0)), 100.0, 100.0, 64.0, 48.0, 96, 128),
    "soup": (lambda: mo.triangle_soup(300, seed=1), _mv(), 80.0, 80.0, 64.0, 48.0, 96, 128),
    "close_up": (lambda: mo.triangle_soup(400, seed=2, center=(0.0, 0.0, -5.0), spread=7.0, size=1.5), _mv(), 60.0, 60.0, 48.0, 48.0, 96, 96),
}
# the ray-cast scenes: the bunny stand-in under four of the views of tests/test_gpu_mesh_rays.py, one per lens
RAY_VIEWS = ("pinhole_1_531x397", "opencv_2_640x480", "fisheye_4_512", "equirect_512x256")
GAP = 1e-4   # the relative depth gap below which the front triangle is not well defined (tests/test_gpu_mesh_color.py)


def raster_flags(v, f, mv, fx, fy, cx, cy, H, W, cull=True):
    """-> (tri, bary, ok [H,W]: not flagged, covered [H,W]) for a raster scene: flagged = ambiguous or grazing by tests/mesh_oracle.py
    (centre within its normalised edge distance of a possibly-front triangle, at a clip plane) or a depth gap below GAP."""
    tri, _, bary, gap = mco.raster_front(v, f, mv, fx, fy, cx, cy, H, W, cull=cull)
    _, amb, graze = mo.raster_depth(v, f, mv, fx, fy, cx, cy, H, W, cull=cull)
    return tri, bary, ~amb & ~graze & (gap > GAP), tri >= 0


def ray_flags(origins, directions, forward, world, f, cull=True):
    """-> (tri [n], bary [n,3], ok [n]: not edge-flagged, z [n]) for a ray-cast scene."""
    z, tri, edge, _ = mro.cast(origins, directions, forward, world, f, cull=cull)
    return tri, hit_barycentrics(origins, directions, world, f, tri), ~(edge < mro.EPS), z
