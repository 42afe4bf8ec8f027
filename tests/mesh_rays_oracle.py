"""Test-only reference of the lens-aware proxy mesh (``sn_mesh_cast_rays``; nothing under signerf_amd/ imports this module).

``cast``: brute force, every ray against every triangle, Moeller-Trumbore in float64 (numpy) from the fp32 rays the GPU gets.  For the
rays of one origin the triangle-only factors of Moeller-Trumbore are hoisted (with T = O - A, e1 = B - A, e2 = C - A, n = e1 x e2:
det = e1 . (d x e2) = -(d . n), u = d . (e2 x T) / det, v = d . (T x e1) / det, t = (T . n) / det), which turns the ray loop into three
matrix products; rays are grouped by origin, so bundles with several origins work too.

Per ray it returns the z-depth (t * (d . forward), 0 where nothing is drawn), the hit triangle (-1) and an EDGE DISTANCE: the smallest
|min(u, v, 1 - u - v)| over the triangles that could be the answer -- drawable ones (in front of the ray's origin, inside the loosened
depth range, front-facing or edge-on when culling) at or before the closest hit's depth * (1 + 1e-4), or any drawable one when the ray
hits nothing (distances of NEAR = 0.01 and more outside a triangle are not resolved: inf).  A ray is EDGE-FLAGGED for eps when that distance is below eps: fp32 cannot be expected to reproduce its answer.  The
distance is 0 for a hit within 1e-5 (relative) of the near / far plane and for a ray within 1e-6 of the plane of a triangle it crosses.

``dtype=np.float32`` runs the same arithmetic in fp32: the "float32 copy of itself" from which tests/test_mesh_rays_host.py derives eps.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import mesh_oracle as mo

REL_DEPTH = 1e-4   # candidates up to this far (relative) behind the closest hit count for the edge distance
PLANE_REL = 1e-5   # |z - znear| <= PLANE_REL * znear (and the same at zfar): at the plane
GRAZE = 1e-6       # |det| <= GRAZE * |n| * |d|: the ray lies in the triangle's plane
NEAR = 0.01        # edge distances are resolved below this; a ray farther than this outside every candidate gets inf


def bumpy_sphere(subdivisions: int = 4, amplitude: float = 0.18):
    """The bunny's stand-in: mesh_oracle.icosphere (F = 20 * 4**subdivisions; 5 120 at 4, the bunny has 4 968) with a radius that depends on
    the direction -- bumps and hollows, so that the silhouette is not a circle and parts of the surface hide others.  The radius is a
    function of the vertex position, so shared edges keep bit-identical endpoints: the surface stays closed.
    -> (vertices [V,3] float32, triangles [F,3] int32, colors [V,3] float in [0, 1], a smooth function of the position)."""
    v, f = mo.icosphere(subdivisions)
    p = v.astype(np.float64)
    r = 1.0 + amplitude * np.sin(3.0 * p[:, 0] + 1.0) * np.sin(4.0 * p[:, 1]) * np.cos(2.0 * p[:, 2] + 0.5)
    col = 0.5 + 0.5 * np.stack([np.sin(2.0 * p[:, 0]), np.cos(3.0 * p[:, 1]), np.sin(2.5 * p[:, 2] + 1.0)], 1)
    return (p * r[:, None]).astype(np.float32), f, np.clip(col, 0.0, 1.0)


def _cast_group(o, D, fwd, A, B, Cc, znear, zfar, cull, dt, chunk, workers):
    e1, e2, T = B - A, Cc - A, o[None, :] - A
    n = np.cross(e1, e2)
    P, Q, tn = np.cross(e2, T), np.cross(T, e1), (T * n).sum(1)
    nn = np.sqrt((n * n).sum(1))
    m = D.shape[0]
    z_out, tri_out, edge_out = np.zeros(m, dtype=np.float64), np.full(m, -1, dtype=np.int64), np.full(m, np.inf)

    def work(s):
        d = D[s:s + chunk]
        f = (d @ fwd).astype(dt)
        dn = np.sqrt((d * d).sum(1))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            det = -(d @ n.T)
            inv = 1.0 / det
            u = (d @ P.T) * inv
            v = (d @ Q.T) * inv
            mn = np.minimum(np.minimum(u, v), 1.0 - u - v)
            # the rest only for the triangles some ray of the chunk comes near (every ray has met every triangle above): beyond NEAR the
            # triangle is neither hit nor a candidate for an edge distance below NEAR
            cols = np.nonzero((mn > -NEAR).any(axis=0))[0]
            det, mn, t = det[:, cols], mn[:, cols], tn[None, cols] * inv[:, cols]
            z = t * f[:, None]
            ahead = (t > 0) & (f[:, None] > 0)
            facing = (det > 0) if cull else (det != 0)
            hit = ahead & facing & (z > znear) & (z < zfar) & (mn >= 0)
            th = np.where(hit, t, np.inf)
            rows = np.arange(d.shape[0])
            if cols.size:
                k = np.argmin(th, axis=1)   # (the first, i.e. the lowest index, of equal distances: cols is ascending)
                best = th[rows, k]
            else:
                k, best = np.zeros(d.shape[0], dtype=np.int64), np.full(d.shape[0], np.inf)
            got = np.isfinite(best)
            # the edge distance
            graze = np.abs(det) <= GRAZE * nn[None, cols] * dn[:, None]
            loose = ahead & (z > znear * (1 - PLANE_REL)) & (z < zfar * (1 + PLANE_REL)) & ((det > 0) | graze if cull else True)
            cand = loose & (mn > -NEAR) & (t <= np.where(got, best * (1 + REL_DEPTH), np.inf)[:, None])
            dist = np.where(cand, np.abs(mn), np.inf)
            at_plane = (np.abs(z - znear) <= PLANE_REL * znear) | (np.abs(z - zfar) <= PLANE_REL * zfar)
            dist = np.where(cand & (at_plane | graze), 0.0, dist)
            edge = dist.min(axis=1) if cols.size else np.full(d.shape[0], np.inf)
        z_out[s:s + chunk] = np.where(got, z[rows, k], 0.0) if cols.size else 0.0
        tri_out[s:s + chunk] = np.where(got, cols[k], -1) if cols.size else -1
        edge_out[s:s + chunk] = edge

    starts = range(0, m, chunk)
    if workers > 1:
        with ThreadPoolExecutor(workers) as ex:
            list(ex.map(work, starts))
    else:
        for s in starts:
            work(s)
    return z_out, tri_out, edge_out


def cast(origins, directions, forward, vertices, triangles, znear=1e-4, zfar=10.0, cull=True, dtype=np.float64, chunk=256, workers=None):
    """origins, directions [..., 3] (the fp32 rays), forward [3], vertices [V,3] (posed, fp32), triangles [F,3]
    -> (z [n] float64, triangle [n] int64, edge distance [n] float64, f = direction . forward [n]), n = the number of rays, row-major."""
    dt = np.dtype(dtype)
    O = np.asarray(origins, dtype=np.float32).reshape(-1, 3).astype(dt)
    D = np.asarray(directions, dtype=np.float32).reshape(-1, 3).astype(dt)
    fwd = np.asarray(forward, dtype=np.float64)
    fwd = (fwd / np.linalg.norm(fwd)).astype(np.float32).astype(dt)
    V = np.asarray(vertices, dtype=np.float32).astype(dt)
    T = np.asarray(triangles, dtype=np.int64)
    A, B, Cc = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    if workers is None:
        workers = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    n = O.shape[0]
    z, tri, edge = np.zeros(n), np.full(n, -1, dtype=np.int64), np.full(n, np.inf)
    uniq, inverse = np.unique(O, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    for g in range(uniq.shape[0]):
        sel = np.nonzero(inverse == g)[0] if uniq.shape[0] > 1 else slice(None)
        z[sel], tri[sel], edge[sel] = _cast_group(uniq[g], D[sel], fwd, A, B, Cc, dt.type(znear), dt.type(zfar), cull, dt, chunk, workers)
    return z, tri, edge, (D.astype(np.float64) @ fwd.astype(np.float64))


def posed(vertices, pose):
    """Object-space vertices -> world space fp32, as Renderer.setup poses them (float64 product, rounded once)."""
    pose = np.asarray(pose, dtype=np.float64)
    return (np.asarray(vertices, dtype=np.float64) @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)


def flagged_shares(flag, covered):
    """(share of the pixels, share of the covered pixels) that are flagged -- the two figures the caps of the GPU tests bound."""
    flag, covered = np.asarray(flag).reshape(-1), np.asarray(covered).reshape(-1)
    return float(flag.mean()), float(flag.sum() / max(int(covered.sum()), 1))


MAX_FLAGGED_OF_PIXELS, MAX_FLAGGED_OF_COVERED = 0.005, 0.05
# derived in the docstring of tests/test_mesh_rays_host.py: a ray is edge-flagged when its edge distance is below EPS; off the flags a
# depth is right when it is within Z_RTOL (relative) of the float64 one
EPS, Z_RTOL = 1.2e-5, 5.6e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# the views of tests/test_gpu_mesh_rays.py (their flagged shares and coverage are verified on the CPU by tests/test_mesh_rays_host.py)
# ---------------------------------------------------------------------------------------------------------------------------------
BUNNY_SCALE = [0.015, 0.015, 0.015]   # x 10 (NERFSTUDIO_BLENDER_SCALE_RATIO): the unit mesh at radius 0.15, about the bunny's extent
PERSPECTIVE, FISHEYE, EQUIRECTANGULAR = 1, 2, 3
OPENCV_DISTORTION = [-0.2, 0.05, 0.0, 0.0, 0.001, -0.002]   # k1 k2 k3 k4 p1 p2


def _look(eye, forward, up=(0.0, 0.0, 1.0)):
    """camera-to-world [3,4] float32 of a nerfstudio camera (x right, y up, looking down -z) at `eye` looking along `forward`."""
    f = np.asarray(forward, dtype=np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, dtype=np.float64))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    return np.concatenate([np.stack([r, u, -f], 1), np.asarray(eye, dtype=np.float64).reshape(3, 1)], 1).astype(np.float32)


def views():
    """name -> dict(c2w [3,4] float32, fx, fy, cx, cy, W, H, distortion (6 floats or None), camera_type).  The pinhole views are three of
    circle_poses(8, radius 0.5) -- the GUI-default reference cameras -- at 800 x 800 and one odd size; the lens views look at the mesh
    from the same circle (OPENCV distortion, FISHEYE) and, for EQUIRECTANGULAR, from 0.19 beside it with the viewing axis at right
    angles to the mesh's direction, so that half of the mesh lies behind the camera."""
    from signerf_amd import scene

    c2w = scene.benchmark_cameras(8)[:, :3].numpy().astype(np.float32)
    out = {}
    for k in (0, 3, 5):
        out[f"pinhole_{k}_800"] = dict(c2w=c2w[k], fx=960.0, fy=960.0, cx=400.0, cy=400.0, W=800, H=800, distortion=None, camera_type=PERSPECTIVE)
    out["pinhole_1_531x397"] = dict(c2w=c2w[1], fx=610.0, fy=640.0, cx=262.3, cy=200.9, W=531, H=397, distortion=None, camera_type=PERSPECTIVE)
    out["opencv_2_640x480"] = dict(c2w=c2w[2], fx=620.0, fy=620.0, cx=320.0, cy=240.0, W=640, H=480, distortion=OPENCV_DISTORTION,
                                   camera_type=PERSPECTIVE)
    out["fisheye_4_512"] = dict(c2w=c2w[4], fx=300.0, fy=300.0, cx=256.0, cy=256.0, W=512, H=512, distortion=None, camera_type=FISHEYE)
    out["equirect_512x256"] = dict(c2w=_look((0.19, 0.0, 0.0), (0.0, 1.0, 0.0)), fx=256.0, fy=256.0, cx=256.0, cy=128.0, W=512, H=256,
                                   distortion=None, camera_type=EQUIRECTANGULAR)
    return out


def cpu_rays(view):
    """The view's rays from the CPU restatement of the ray generation (oracle/nerfacto.py) -> (origins, directions) [H,W,3] float32."""
    import torch

    from oracle import nerfacto as onf

    d = None if view["distortion"] is None else torch.tensor(view["distortion"], dtype=torch.float32)
    r = onf.generate_rays(torch.from_numpy(view["c2w"]), view["fx"], view["fy"], view["cx"], view["cy"], view["H"], view["W"], d, view["camera_type"])
    return r["origins"].numpy(), r["directions"].numpy()


def forward_of(c2w):
    return -np.asarray(c2w, dtype=np.float64)[:3, 2]
