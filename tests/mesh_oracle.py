"""Test-only references of the shape masking mode (nothing under signerf_amd/ imports this module):

* ``raster_depth``: a float64 numpy restatement of what pyrender's depth buffer holds at a pixel centre -- the smallest eye z-depth in
  [znear, zfar] over the triangles whose projection covers the centre, GL_BACK culling with counter-clockwise front faces, 0 elsewhere.
  It also reports, per pixel, whether the answer is numerically AMBIGUOUS (the centre lies within ``eps`` -- a normalised angular
  distance -- of an edge of a triangle that could be the front one, or at the near / far plane, or on a triangle seen edge-on so that
  its culling is a coin toss) and whether the front hit is GRAZING (the ray nearly in the triangle's plane: its depth is ill-conditioned).
* ``shape_mask_and_condition``: datasetgenerator.py:716-754 restated on CPU fp32 tensors, operation for operation.
* procedural meshes: icospheres, quads, random triangle soup.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import signerf_utils as su


# ---------------------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions: int, radius: float = 1.0):
    """-> (vertices [V,3] float32, triangles [F,3] int32), F = 20 * 4**subdivisions, faces counter-clockwise seen from outside.  The
    vertices are per face (a triangle soup: V = 3F); shared edges have bit-identical endpoints, so the surface is closed."""
    t = (1.0 + 5 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    tri = v[f]  # [F,3,3]
    for _ in range(subdivisions):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = a + b, b + c, c + a
        ab /= np.linalg.norm(ab, axis=1, keepdims=True)
        bc /= np.linalg.norm(bc, axis=1, keepdims=True)
        ca /= np.linalg.norm(ca, axis=1, keepdims=True)
        tri = np.stack([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)], 1).reshape(-1, 3, 3)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    flip = (n * tri.sum(1)).sum(1) < 0
    tri[flip] = tri[flip][:, [0, 2, 1]]
    verts = (tri.reshape(-1, 3) * radius).astype(np.float32)
    return verts, np.arange(verts.shape[0], dtype=np.int32).reshape(-1, 3)


def quad(x0, x1, y0, y1, z, ccw_towards=+1):
    """Axis-aligned rectangle in the plane z, two triangles whose front face looks along +z (ccw_towards=+1) or -z."""
    v = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    if ccw_towards < 0:
        f = f[:, [0, 2, 1]]
    return v, f


def triangle_soup(n: int, seed: int, center=(0.0, 0.0, -3.0), spread=1.5, size=0.4):
    g = np.random.default_rng(seed)
    c = np.asarray(center) + g.uniform(-spread, spread, size=(n, 1, 3))
    v = (c + g.uniform(-size, size, size=(n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 rasteriser
# ---------------------------------------------------------------------------------------------------------------------------------
def _norm(x):
    return np.sqrt((x * x).sum(-1))


def raster_depth(vertices, triangles, mv, fx, fy, cx, cy, H, W, znear=1e-4, zfar=10.0, cull=True, eps=1e-5, graze=1e-3, chunk=200_000):
    """-> (depth [H,W] float64, ambiguous [H,W] bool, grazing [H,W] bool).  mv: camera-from-object [3,4]."""
    mv = np.asarray(mv, dtype=np.float64).reshape(3, 4)
    V = np.asarray(vertices, dtype=np.float64) @ mv[:, :3].T + mv[:, 3]
    T = np.asarray(triangles, dtype=np.int64)
    best = np.full(H * W, np.inf)
    best_graze = np.zeros(H * W, dtype=bool)
    amb_t = np.full(H * W, np.inf)  # nearest t of an ambiguous candidate
    for s in range(0, T.shape[0], chunk):
        A, B, Cc = V[T[s:s + chunk, 0]], V[T[s:s + chunk, 1]], V[T[s:s + chunk, 2]]
        E = np.stack([np.cross(B, Cc), np.cross(Cc, A), np.cross(A, B)], 1)  # [f,3,3]
        n = np.cross(B - A, Cc - A)
        nA = (n * A).sum(-1)
        z = -np.stack([A[:, 2], B[:, 2], Cc[:, 2]], 1)
        out = (z < znear).all(1) | (z > zfar).all(1)
        edge_on = np.abs(nA) <= eps * _norm(n) * _norm(A)
        keep = (~out & ((nA < 0) | edge_on)) if cull else ~out
        idx = np.nonzero(keep)[0]
        if idx.size == 0:
            continue
        # pixel-centre bbox, padded by 0.05 px (whole image for a triangle that reaches the camera plane)
        zz = z[idx]
        front = (zz > 0).all(1)
        P = np.stack([A[idx], B[idx], Cc[idx]], 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = fx * P[..., 0] / np.where(front[:, None], zz, 1.0) + cx
            w = -fy * P[..., 1] / np.where(front[:, None], zz, 1.0) + cy
        j0 = np.where(front, np.ceil(u.min(1) - 0.5 - 0.05), 0).clip(0, W).astype(np.int64)
        j1 = np.where(front, np.floor(u.max(1) - 0.5 + 0.05), W - 1).clip(-1, W - 1).astype(np.int64)
        i0 = np.where(front, np.ceil(w.min(1) - 0.5 - 0.05), 0).clip(0, H).astype(np.int64)
        i1 = np.where(front, np.floor(w.max(1) - 0.5 + 0.05), H - 1).clip(-1, H - 1).astype(np.int64)
        nw, nh = np.maximum(j1 - j0 + 1, 0), np.maximum(i1 - i0 + 1, 0)
        cnt = nw * nh
        tri = np.repeat(np.arange(idx.size), cnt)
        if tri.size == 0:
            continue
        local = np.arange(tri.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        pi = i0[tri] + local // nw[tri]
        pj = j0[tri] + local % nw[tri]
        d = np.stack([(pj + 0.5 - cx) / fx, -(pi + 0.5 - cy) / fy, -np.ones(pj.shape)], -1)
        g = idx[tri]
        e = (E[g] * d[:, None, :]).sum(-1) / np.maximum(_norm(E[g]) * _norm(d)[:, None], 1e-300)
        inside = (e >= 0).all(1) | (e <= 0).all(1)
        near = (e >= -eps).all(1) | (e <= eps).all(1)
        nd = (n[g] * d).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = nA[g] / nd
        in_range = (t >= znear) & (t <= zfar)
        near_range = (t >= znear * (1 - 1e-5)) & (t <= zfar * (1 + 1e-5))
        at_plane = near_range & ((np.abs(t - znear) <= 1e-5 * znear) | (np.abs(t - zfar) <= 1e-5 * zfar))
        valid = inside & in_range & ~(edge_on[g] & cull)
        amb = near & near_range & ((np.abs(e).min(1) < eps) | at_plane | edge_on[g])
        pix = pi * W + pj
        gr = np.abs(nd) < graze * _norm(n[g]) * _norm(d)
        # nearest valid hit per pixel (ties keep the smaller t either way)
        tv = np.where(valid, t, np.inf)
        order = np.lexsort((tv, pix))
        ps, ts, gs = pix[order], tv[order], gr[order]
        first = np.ones(ps.size, dtype=bool)
        first[1:] = ps[1:] != ps[:-1]
        ps, ts, gs = ps[first], ts[first], gs[first]
        better = ts < best[ps]
        best[ps[better]] = ts[better]
        best_graze[ps[better]] = gs[better]
        np.minimum.at(amb_t, pix[amb], np.where(np.isfinite(t[amb]), t[amb], 0.0))
    depth = np.where(np.isfinite(best), best, 0.0)
    ambiguous = (amb_t < np.inf) & (amb_t <= np.where(np.isfinite(best), best * (1 + 1e-4), np.inf))
    return depth.reshape(H, W), ambiguous.reshape(H, W), best_graze.reshape(H, W)


# ---------------------------------------------------------------------------------------------------------------------------------
# datasetgenerator.py:716-754, fp32 on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def shape_mask_and_condition(mesh_depth, depth_tensor, mask_dialation=(50, 50), inverse_mask=False, manual_depth=None,
                             additional_depth_radius=0.1):
    """-> (mask [H,W,1] bool, condition [H,W,1] fp32).  The reference's torch.min of an empty selection (something visible, no visible
    pixel with mesh depth > 0) raises; this package defines that condition as all zeros, and so does this restatement."""
    depth = mesh_depth.to(torch.float32)
    depth_tensor = depth_tensor.to(torch.float32)
    H, W = depth.shape[0], depth.shape[1]
    non_empty_space = depth > 0
    visible_mask = (depth < depth_tensor) * non_empty_space
    visible_mask = ~visible_mask if inverse_mask else visible_mask
    if not bool(torch.sum(visible_mask) > 1e-6):
        return torch.zeros(H, W, 1, dtype=torch.bool), torch.zeros(H, W, 1, dtype=torch.float32)
    if mask_dialation is not None:
        vis_np = visible_mask.numpy().astype(float)[..., 0]
        mask_image = torch.tensor(su.dilate(vis_np, su.ellipse_element(*mask_dialation)), dtype=torch.float32).unsqueeze(-1) > 0
    else:
        mask_image = visible_mask
    if manual_depth is not None:
        min_manual_depth, max_manual_depth = manual_depth
    else:
        sel = depth[visible_mask * depth > 0]
        if sel.numel() == 0:
            return mask_image, torch.zeros(H, W, 1, dtype=torch.float32)
        min_manual_depth = torch.min(sel) - additional_depth_radius
        max_manual_depth = torch.max(depth) + additional_depth_radius
    object_depth_normalized = (depth - min_manual_depth) / (max_manual_depth - min_manual_depth)
    nerf_depth_normalized = (depth_tensor - min_manual_depth) / (max_manual_depth - min_manual_depth)
    condition_image = visible_mask * object_depth_normalized + (~visible_mask) * nerf_depth_normalized
    return mask_image, 1 - torch.clamp(condition_image, 0, 1)
