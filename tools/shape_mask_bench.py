#!/usr/bin/env python3
"""Shape masking mode cost per view: proxy-mesh raster (sn_mesh_raster_depth) + shape mask / condition (sn_shape_mask_condition) at
800 x 800, beside the 800 x 800 x 64-sample NeRF render of the same view (scene.benchmark_config(64), the bench.py workload).  Times are
hipEvent intervals on the stream, median of --reps after --warmup.

Meshes (tests/mesh_oracle.py's procedural icosphere restated here: tools do not import the tests):
  bunny_5120    a 5 120-face icosphere of radius 0.15 at the origin (bunny-sized: the bunny has 4 968 faces), seen from the
                benchmark cameras (views 0, 2, 4, 6 of circle_poses(8), radius 0.5)
  closeup_5120  the same mesh 0.12 in front of the camera: its triangles cover large parts of the frame
  big_1.3M      a 1 310 720-face icosphere in the bunny's place

    python tools/shape_mask_bench.py [--size 800] [--reps 50] [--json OUT]

--combine times the aabb mode's combine_shape_with_depth instead (bunny_5120 and closeup_5120): the colour raster
(sn_mesh_raster_color, colour + depth) against the depth raster, and the combined aabb step (sn_aabb_mask_condition_combined) against
the plain one (sn_aabb_mask_condition); flag_share = what the flag adds to a view (colour raster + combined step - plain step) over the
NeRF render.

    python tools/shape_mask_bench.py --combine [--size 800] [--reps 50] [--json OUT]

--rays times the lens-aware proxy mesh (RendererConfig.lens = "camera"): the ray cast of the bunny-sized mesh (sn_mesh_cast_rays, depth
only and colour + depth, over the view's own ray bundle) beside the pinhole raster and the NeRF render of the same view, per view and as
medians; the acceleration structure's host build time and size are reported once.  cast_over_nerf must stay below 1: the generator
keeps two frames in flight, so a mask step longer than the render would bound the view loop.

    python tools/shape_mask_bench.py --rays [--size 800] [--reps 50] [--json OUT]

--materials times the proxy-mesh materials (RendererConfig.materials = "mtl"): the textured colour raster (sn_mesh_raster_color_materials:
three materials over thirds of the mesh, a 64 x 64 and a 96 x 40 texture, spherical uv) beside the depth raster and the colour raster
without and with vertex colours, for bunny_5120 and closeup_5120, and the textured ray cast (sn_mesh_cast_rays_materials) beside the
vertex-colour ray cast for bunny_5120 (the close-up is a model-view of the raster only).  The vertex-colour path is the nearest
existing one: the same sweep or walk, an epilogue with three gathers instead of about twelve loads.

    python tools/shape_mask_bench.py --materials [--size 800] [--reps 50] [--json OUT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from signerf_amd import Cameras, scene  # noqa: E402
from signerf_amd.datasetgenerator import aabb_mask_and_condition, aabb_mask_and_condition_combined, shape_mask_and_condition  # noqa: E402
from signerf_amd.renderer import RendererConfig, build_accel, cast_rays, model_view, object_pose, raster_color, raster_depth  # noqa: E402


def icosphere(subdivisions):
    t = (1.0 + 5 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    tri = v[f]
    for _ in range(subdivisions):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = a + b, b + c, c + a
        for m in (ab, bc, ca):
            m /= np.linalg.norm(m, axis=1, keepdims=True)
        tri = np.stack([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)], 1).reshape(-1, 3, 3)
    verts = tri.reshape(-1, 3).astype(np.float32)
    return verts, np.arange(verts.shape[0], dtype=np.int32).reshape(-1, 3)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nerf-reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--combine", action="store_true", help="time combine_shape_with_depth (see the module docstring)")
    ap.add_argument("--rays", action="store_true", help="time the lens-aware ray cast beside the raster and the NeRF render")
    ap.add_argument("--materials", action="store_true", help="time the textured colour raster and ray cast beside the vertex-colour ones")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    S = a.size
    cfg = scene.benchmark_config(64)
    model = cfg.setup()
    model.load_state_dict(scene.synthetic_state_dict(cfg, seed=0), strict=False)
    model = model.to(dev).eval()
    c2w = scene.benchmark_cameras(8)[:, :3]
    cams = Cameras(c2w, 1.2 * S, 1.2 * S, S / 2, S / 2, S, S).to(dev)
    pose = object_pose(RendererConfig(scale=[0.015, 0.015, 0.015]))   # radius 0.15, about the bunny's extent at the default scale
    if a.combine:
        return combine(a, model, cams, pose, dev)
    if a.rays:
        return rays(a, model, cams, pose, dev)
    if a.materials:
        return materials(a, model, cams, pose, dev)
    meshes = {"bunny_5120": icosphere(4), "big_1.3M": icosphere(8)}
    rows = []
    for view in range(0, 8, 2):
        cam = cams[view]
        bundle = cam.generate_rays(0, aabb_box=model.render_aabb)
        nerf_ms = timed(lambda: model.get_outputs_for_camera_ray_bundle(bundle), a.nerf_reps, 2)
        nerf_depth = model.get_outputs_for_camera_ray_bundle(bundle)["depth"]
        host = cam._host[0].tolist()
        legs = [("bunny_5120", model_view(host[:12], pose)), ("big_1.3M", model_view(host[:12], pose))]
        # close-up: the same mesh 0.12 in front of the camera (radius 0.15: the camera sits just outside it, the frame is mostly mesh)
        close = model_view(host[:12], pose).copy()
        close[:, 3] = [0.0, 0.0, -0.27]
        legs.append(("closeup_5120", close))
        for name, mv in legs:
            v, f = meshes["big_1.3M" if name.startswith("big") else "bunny_5120"]
            vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
            depth = torch.empty((S, S, 1), device=dev)
            r_ms = timed(lambda: raster_depth(vt, ft, mv, host[12], host[13], host[14], host[15], S, S, out=depth), a.reps, a.warmup)
            m_ms = timed(lambda: shape_mask_and_condition(depth, nerf_depth), a.reps, a.warmup)
            cover = float((depth > 0).float().mean())
            rows.append({"view": view, "mesh": name, "faces": int(f.shape[0]), "raster_ms": round(r_ms, 4), "mask_ms": round(m_ms, 4),
                         "raster_plus_mask_ms": round(r_ms + m_ms, 4), "nerf_render_ms": round(nerf_ms, 3),
                         "share_of_render": round((r_ms + m_ms) / nerf_ms, 4), "mesh_coverage": round(cover, 4)})
            print(json.dumps(rows[-1]), flush=True)
    summary = {}
    for name in ("bunny_5120", "closeup_5120", "big_1.3M"):
        rs = [r for r in rows if r["mesh"] == name]
        summary[name] = {k: float(np.median([r[k] for r in rs])) for k in ("raster_ms", "mask_ms", "raster_plus_mask_ms", "nerf_render_ms",
                                                                             "share_of_render", "mesh_coverage")}
    out = {"size": S, "reps": a.reps, "gpu": torch.cuda.get_device_name(0), "median_over_views": summary, "rows": rows}
    print(json.dumps({"median_over_views": summary}))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


def combine(a, model, cams, pose, dev):
    S = a.size
    v, f = icosphere(4)
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    box = torch.tensor([[-0.1, -0.1, -0.1], [0.1, 0.1, 0.1]])   # DatasetGeneratorConfig's default aabb
    rows = []
    for view in range(0, 8, 2):
        cam = cams[view]
        bundle = cam.generate_rays(0, aabb_box=model.render_aabb)
        nerf_ms = timed(lambda: model.get_outputs_for_camera_ray_bundle(bundle), a.nerf_reps, 2)
        nerf_depth = model.get_outputs_for_camera_ray_bundle(bundle)["depth"]
        o, d = bundle.origins.contiguous(), bundle.directions.contiguous()
        host = cam._host[0].tolist()
        close = model_view(host[:12], pose).copy()
        close[:, 3] = [0.0, 0.0, -0.27]
        for name, mv in (("bunny_5120", model_view(host[:12], pose)), ("closeup_5120", close)):
            intr = (host[12], host[13], host[14], host[15], S, S)
            d_ms = timed(lambda: raster_depth(vt, ft, mv, *intr), a.reps, a.warmup)
            c_ms = timed(lambda: raster_color(vt, ft, mv, *intr), a.reps, a.warmup)
            color, md = raster_color(vt, ft, mv, *intr)
            p_ms = timed(lambda: aabb_mask_and_condition(nerf_depth, o, d, box), a.reps, a.warmup)
            k_ms = timed(lambda: aabb_mask_and_condition_combined(nerf_depth, o, d, box, md, color), a.reps, a.warmup)
            cv = float(((md > 0) & (md < nerf_depth)).float().mean())
            rows.append({"view": view, "mesh": name, "faces": int(f.shape[0]), "depth_raster_ms": round(d_ms, 4), "color_raster_ms": round(c_ms, 4),
                         "color_over_depth": round(c_ms / d_ms, 4), "plain_aabb_ms": round(p_ms, 4), "combined_aabb_ms": round(k_ms, 4),
                         "combined_minus_plain_ms": round(k_ms - p_ms, 4), "nerf_render_ms": round(nerf_ms, 3),
                         "flag_share": round((c_ms + k_ms - p_ms) / nerf_ms, 4), "mesh_coverage": round(float((md > 0).float().mean()), 4),
                         "mesh_in_front": round(cv, 4)})
            print(json.dumps(rows[-1]), flush=True)
    keys = ("depth_raster_ms", "color_raster_ms", "color_over_depth", "plain_aabb_ms", "combined_aabb_ms", "combined_minus_plain_ms",
            "nerf_render_ms", "flag_share", "mesh_coverage", "mesh_in_front")
    summary = {name: {k: float(np.median([r[k] for r in rows if r["mesh"] == name])) for k in keys} for name in ("bunny_5120", "closeup_5120")}
    out = {"size": S, "reps": a.reps, "gpu": torch.cuda.get_device_name(0), "leg": "combine", "median_over_views": summary, "rows": rows}
    print(json.dumps({"median_over_views": summary}))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


def rays(a, model, cams, pose, dev):
    import time

    S = a.size
    v, f = icosphere(4)
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    world = (v.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)
    t0 = time.perf_counter()
    blob = build_accel(world, f)
    build_s = time.perf_counter() - t0
    accel = torch.from_numpy(blob).to(dev)
    rows = []
    for view in range(0, 8, 2):
        cam = cams[view]
        bundle = cam.generate_rays(0, aabb_box=model.render_aabb)
        nerf_ms = timed(lambda: model.get_outputs_for_camera_ray_bundle(bundle), a.nerf_reps, 2)
        o, d = bundle.origins.contiguous(), bundle.directions.contiguous()
        host = cam._host[0].tolist()
        fwd = (-host[2], -host[6], -host[10])
        mv = model_view(host[:12], pose)
        intr = (host[12], host[13], host[14], host[15], S, S)
        r_ms = timed(lambda: raster_depth(vt, ft, mv, *intr), a.reps, a.warmup)
        rc_ms = timed(lambda: raster_color(vt, ft, mv, *intr), a.reps, a.warmup)
        c_ms = timed(lambda: cast_rays(o, d, fwd, accel, f.shape[0], S, S), a.reps, a.warmup)
        cc_ms = timed(lambda: cast_rays(o, d, fwd, accel, f.shape[0], S, S, ft, None, v.shape[0], with_color=True), a.reps, a.warmup)
        zc, zr = cast_rays(o, d, fwd, accel, f.shape[0], S, S)[1], raster_depth(vt, ft, mv, *intr)
        rows.append({"view": view, "mesh": "bunny_5120", "faces": int(f.shape[0]), "raster_ms": round(r_ms, 4), "raster_color_ms": round(rc_ms, 4),
                     "cast_ms": round(c_ms, 4), "cast_color_ms": round(cc_ms, 4), "nerf_render_ms": round(nerf_ms, 3),
                     "cast_over_raster": round(c_ms / r_ms, 3), "cast_over_nerf": round(c_ms / nerf_ms, 4),
                     "mesh_coverage": round(float((zc > 0).float().mean()), 4),
                     "coverage_differs_px": int(((zc > 0) != (zr > 0)).sum())})
        print(json.dumps(rows[-1]), flush=True)
    keys = ("raster_ms", "raster_color_ms", "cast_ms", "cast_color_ms", "nerf_render_ms", "cast_over_raster", "cast_over_nerf", "mesh_coverage")
    summary = {"bunny_5120": {k: float(np.median([r[k] for r in rows])) for k in keys}}
    out = {"size": S, "reps": a.reps, "gpu": torch.cuda.get_device_name(0), "leg": "rays", "accel_build_host_s": round(build_s, 4),
           "accel_bytes": int(blob.size), "median_over_views": summary, "rows": rows}
    print(json.dumps({"accel_build_host_s": out["accel_build_host_s"], "accel_bytes": out["accel_bytes"], "median_over_views": summary}))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


def _bench_materials(v, f):
    """Three materials over thirds of the mesh (two textured, one Kd only), spherical per-corner uv that cross the wrap seam, and
    position-dependent vertex colours for the path it is compared with."""
    from signerf_amd.renderer import ObjMaterial, pack_materials

    def texture(w, h, seed):
        x, y = np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h)
        t = np.full((h, w, 4), 255, dtype=np.uint8)
        for c in range(3):
            t[..., c] = np.round(255 * (0.2 + 0.8 * (0.5 + 0.5 * np.sin(2 * np.pi * ((1 + c % 2) * x + y) + c + seed)))).astype(np.uint8)
        return t

    p = v.astype(np.float64)
    r = np.maximum(np.linalg.norm(p, axis=1), 1e-12)
    cu = (np.arctan2(p[:, 1], p[:, 0]) / (2 * np.pi) + 0.5)[f]
    cw = (1.0 - np.arccos(np.clip(p[:, 2] / r, -1, 1)) / np.pi)[f]
    cu = np.where((cu.max(1, keepdims=True) - cu) > 0.5, cu + 1.0, cu)
    uv = np.stack([cu, cw], -1).astype(np.float32)
    tm = np.minimum(np.arange(f.shape[0]) * 3 // f.shape[0], 2).astype(np.int32)
    mats = [ObjMaterial("square", (0.9, 0.8, 1.0), "a", texture(64, 64, 0)), ObjMaterial("oblong", (1.0, 1.0, 1.0), "b", texture(96, 40, 1)),
            ObjMaterial("plain", (0.55, 0.35, 0.75))]
    vc = np.full((v.shape[0], 4), 255, dtype=np.uint8)
    vc[:, :3] = np.round(255 * (0.2 + 0.8 * (0.5 + 0.5 * np.sin(3.0 * p + 0.5)))).astype(np.uint8)
    return pack_materials(uv, tm, mats), vc


def materials(a, model, cams, pose, dev):
    from signerf_amd.renderer import cast_rays_materials, raster_color_materials

    S = a.size
    v, f = icosphere(4)
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    mm, vc = _bench_materials(v, f)
    vct = torch.from_numpy(vc).to(dev)
    world = (v.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)
    accel = torch.from_numpy(build_accel(world, f)).to(dev)
    white = (1.0, 1.0, 1.0, 1.0)
    rows = []
    for view in range(0, 8, 2):
        cam = cams[view]
        bundle = cam.generate_rays(0, aabb_box=model.render_aabb)
        o, d = bundle.origins.contiguous(), bundle.directions.contiguous()
        host = cam._host[0].tolist()
        fwd = (-host[2], -host[6], -host[10])
        close = model_view(host[:12], pose).copy()
        close[:, 3] = [0.0, 0.0, -0.27]
        intr = (host[12], host[13], host[14], host[15], S, S)
        for name, mv in (("bunny_5120", model_view(host[:12], pose)), ("closeup_5120", close)):
            row = {"view": view, "mesh": name, "faces": int(f.shape[0]),
                   "raster_depth_ms": round(timed(lambda: raster_depth(vt, ft, mv, *intr), a.reps, a.warmup), 4),
                   "raster_color_ms": round(timed(lambda: raster_color(vt, ft, mv, *intr), a.reps, a.warmup), 4),
                   "raster_vertex_color_ms": round(timed(lambda: raster_color(vt, ft, mv, *intr, vct, base_color=white), a.reps, a.warmup), 4),
                   "raster_materials_ms": round(timed(lambda: raster_color_materials(vt, ft, mv, *intr, mm), a.reps, a.warmup), 4)}
            if name == "bunny_5120":
                row["cast_vertex_color_ms"] = round(timed(lambda: cast_rays(o, d, fwd, accel, f.shape[0], S, S, ft, vct, v.shape[0], with_color=True,
                                                                            base_color=white), a.reps, a.warmup), 4)
                row["cast_materials_ms"] = round(timed(lambda: cast_rays_materials(o, d, fwd, accel, f.shape[0], S, S, mm), a.reps, a.warmup), 4)
                row["cast_materials_over_vertex_color"] = round(row["cast_materials_ms"] / row["cast_vertex_color_ms"], 3)
            row["raster_materials_over_vertex_color"] = round(row["raster_materials_ms"] / row["raster_vertex_color_ms"], 3)
            row["mesh_coverage"] = round(float((raster_depth(vt, ft, mv, *intr) > 0).float().mean()), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
    summary = {}
    for name in ("bunny_5120", "closeup_5120"):
        sel = [r for r in rows if r["mesh"] == name]
        summary[name] = {k: float(np.median([r[k] for r in sel])) for k in sel[0] if k.endswith("_ms") or k.endswith("_color") or k == "mesh_coverage"}
    out = {"size": S, "reps": a.reps, "gpu": torch.cuda.get_device_name(0), "leg": "materials", "median_over_views": summary, "rows": rows}
    print(json.dumps({"median_over_views": summary}))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
