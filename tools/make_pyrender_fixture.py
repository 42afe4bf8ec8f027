#!/usr/bin/env python3
"""Emit golden fixtures from the REAL pyrender + trimesh -- to be run wherever `pip install pyrender trimesh` works and an offscreen GL
context can be made (EGL or OSMesa; it is not available in the build container nor on the GPU box).  It pins what is unpinned today: the
shading constants of signerf_amd/renderer.py (pyrender's default material 0.3 grey, baseColorFactor 1 with vertex colours, the
pow(1/2.2) output, the white clear colour) that ``combine_shape_with_depth`` pastes into the aabb condition
(/root/reference/signerf/renderer/renderer.py:64-196, datasetgenerator.py:794-811).

  tests/golden/pyrender/ico_plain.npz     a procedural icosphere (no visuals) in a Scene(ambient_light=[1, 1, 1]) with no other light,
                                          rendered through an IntrinsicsCamera(znear=1e-4, zfar=10) as the reference renders its mesh
  tests/golden/pyrender/ico_colored.npz   the same mesh with position-dependent vertex colours

Each file holds the inputs (vertices, triangles, vertex_colors (empty when none), model_view [3,4] camera-from-object, intrinsics
fx fy cx cy) and pyrender's outputs (color [H,W,3] uint8, depth [H,W] fp32).  Only inputs and outputs are stored -- no pyrender source.

THE RECIPE (any machine with network access and a GL driver; CPU is enough):

    python3.10 -m venv /tmp/pr && . /tmp/pr/bin/activate
    pip install numpy torch pyrender trimesh pytest
    PYOPENGL_PLATFORM=egl python tools/make_pyrender_fixture.py          # (or PYOPENGL_PLATFORM=osmesa)
    python -m pytest tests/test_mesh_color_host.py -k pyrender_fixture    # the consumer test, skipped until the files exist
    git add tests/golden/pyrender/*.npz

Expected size: ~60 KB per file at the default 96 x 128.

--materials writes instead the two fixtures that pin ``signerf_amd.renderer.material_defaults`` (texture_srgb, the default material of a
face without usemtl, vertex colours dropped once a material resolves, the Kd of a newmtl without one) and the material shading:

  tests/golden/pyrender_materials/kd.npz        the icosphere as an OBJ + MTL with three Kd-only materials over thirds of the mesh (one
                                                of them without Kd), the first faces before any usemtl, and vertex colours in the file
  tests/golden/pyrender_materials/textured.npz  the same mesh with per-corner vt from a spherical map and a map_Kd texture (64 x 64 PNG)

The OBJ, MTL and PNG are written to a temporary directory and loaded with ``trimesh.load`` as the reference loads its mesh; each file holds
the mesh as this package reads it (vertices, triangles, corner_uv, triangle_material, kd [M,3] (NaN: none in the file), texture_k), the
camera, and pyrender's color / depth.  Consumer: tests/test_mesh_material_host.py -k pyrender_fixture.

    PYOPENGL_PLATFORM=egl python tools/make_pyrender_fixture.py --materials
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pyrender")


def icosphere(subdivisions, radius=1.0):
    """Faces counter-clockwise seen from outside, one vertex per corner (tests/mesh_oracle.py's mesh, restated: tools do not import tests)."""
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
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    flip = (n * tri.sum(1)).sum(1) < 0
    tri[flip] = tri[flip][:, [0, 2, 1]]
    verts = (tri.reshape(-1, 3) * radius).astype(np.float32)
    return verts, np.arange(verts.shape[0], dtype=np.int32).reshape(-1, 3)


def position_colors(vertices, lo=0.2):
    """As tests/mesh_color_oracle.py::position_colors: RGBA8, a function of the position only."""
    v = np.asarray(vertices, dtype=np.float64)
    a = 0.5 + 0.5 * np.sin(np.stack([3.1 * v[:, 0] + 0.7, 2.3 * v[:, 1] - 1.1, 1.7 * v[:, 2] + 2.9 * v[:, 0]], 1))
    rgba = np.full((v.shape[0], 4), 255, dtype=np.uint8)
    rgba[:, :3] = np.round(255.0 * (lo + (1.0 - lo) * a)).astype(np.uint8)
    return rgba


def render(v, f, vc, mv, fx, fy, cx, cy, H, W):
    import pyrender
    import trimesh

    mesh = trimesh.Trimesh(vertices=v, faces=f, vertex_colors=vc, process=False) if vc is not None else \
        trimesh.Trimesh(vertices=v, faces=f, process=False)
    scene = pyrender.Scene(ambient_light=[1.0, 1.0, 1.0])   # renderer.py:130, no other light
    pose = np.eye(4)
    pose[:3] = mv   # the mesh placed in camera space, the camera at the origin looking down -z
    scene.add(pyrender.Mesh.from_trimesh(mesh), pose=pose)
    scene.add(pyrender.IntrinsicsCamera(fx=fx, fy=fy, cx=cx, cy=cy, znear=0.0001, zfar=10), pose=np.eye(4))
    r = pyrender.OffscreenRenderer(viewport_width=W, viewport_height=H)
    try:
        color, depth = r.render(scene)
    finally:
        r.delete()
    return np.ascontiguousarray(color[..., :3]).astype(np.uint8), np.ascontiguousarray(depth).astype(np.float32)


def render_file(obj_path, mv, fx, fy, cx, cy, H, W):
    """As ``render``, for a mesh that trimesh loads from a file with its materials (the reference's ``trimesh.load``)."""
    import pyrender
    import trimesh

    mesh = trimesh.load(obj_path, force="mesh", process=False)
    scene = pyrender.Scene(ambient_light=[1.0, 1.0, 1.0])
    pose = np.eye(4)
    pose[:3] = mv
    scene.add(pyrender.Mesh.from_trimesh(mesh), pose=pose)
    scene.add(pyrender.IntrinsicsCamera(fx=fx, fy=fy, cx=cx, cy=cy, znear=0.0001, zfar=10), pose=np.eye(4))
    r = pyrender.OffscreenRenderer(viewport_width=W, viewport_height=H)
    try:
        color, depth = r.render(scene)
    finally:
        r.delete()
    return np.ascontiguousarray(color[..., :3]).astype(np.uint8), np.ascontiguousarray(depth).astype(np.float32)


def materials_fixtures(out, mv, fx, fy, cx, cy, H, W):
    import tempfile

    from PIL import Image

    sys.path.insert(0, ROOT)
    from signerf_amd.renderer import load_obj, load_obj_materials

    v, f = icosphere(3, 0.5)
    vc = position_colors(v)
    F = f.shape[0]
    tm = np.minimum(np.arange(F) * 3 // F, 2)
    p = v.astype(np.float64)
    cu = (np.arctan2(p[:, 1], p[:, 0]) / (2 * np.pi) + 0.5)[f]
    cw = (1.0 - np.arccos(np.clip(p[:, 2] / np.linalg.norm(p, axis=1), -1, 1)) / np.pi)[f]
    cu = np.where((cu.max(1, keepdims=True) - cu) > 0.5, cu + 1.0, cu)
    x, y = np.meshgrid((np.arange(64) + 0.5) / 64, (np.arange(64) + 0.5) / 64)
    tex = np.full((64, 64, 3), 255, dtype=np.uint8)
    for c in range(3):
        tex[..., c] = np.round(255 * (0.2 + 0.8 * (0.5 + 0.5 * np.sin(2 * np.pi * ((1 + c % 2) * x + y) + c)))).astype(np.uint8)
    os.makedirs(out, exist_ok=True)
    for name, textured in (("kd", False), ("textured", True)):
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "m.mtl"), "w") as fh:
                fh.write("newmtl a\nKd 0.8 0.1 0.05\n" + ("map_Kd t.png\n" if textured else "") + "newmtl b\nKd 0.2 0.6 0.9\nnewmtl c\nNs 10\n")
            if textured:
                Image.fromarray(tex, "RGB").save(os.path.join(d, "t.png"))
            with open(os.path.join(d, "m.obj"), "w") as fh:
                fh.write("mtllib m.mtl\n")
                fh.write("".join(f"v {a:.9g} {b:.9g} {c:.9g} {r / 255:.9g} {g / 255:.9g} {bl / 255:.9g}\n"
                                 for (a, b, c), (r, g, bl, _) in zip(v.tolist(), vc.tolist())))
                if textured:
                    fh.write("".join(f"vt {a:.9g} {b:.9g}\n" for a, b in np.stack([cu, cw], -1).reshape(-1, 2).tolist()))
                last = None
                for k, (a, b, c) in enumerate(f.tolist()):
                    if k >= 8 and tm[k] != last:   # the first eight faces come before any usemtl
                        fh.write(f"usemtl {'abc'[tm[k]]}\n")
                        last = tm[k]
                    fh.write(f"f {a + 1}/{3 * k + 1} {b + 1}/{3 * k + 2} {c + 1}/{3 * k + 3}\n" if textured else f"f {a + 1} {b + 1} {c + 1}\n")
            obj = os.path.join(d, "m.obj")
            color, depth = render_file(obj, mv, fx, fy, cx, cy, H, W)
            hv, hf = load_obj(obj)
            uv, htm, mats = load_obj_materials(obj)
            extra = {f"texture_{k}": m.texture for k, m in enumerate(mats) if m.texture is not None}
            path = os.path.join(out, f"{name}.npz")
            np.savez_compressed(path, vertices=hv, triangles=hf, corner_uv=np.zeros((0, 3, 2), np.float32) if uv is None else uv,
                                triangle_material=htm, kd=np.array([m.kd if m.kd is not None else (np.nan,) * 3 for m in mats], dtype=np.float64),
                                model_view=mv, intrinsics=np.array([fx, fy, cx, cy]), color=color, depth=depth, **extra)
            print(f"{path}: {os.path.getsize(path)} bytes, {int((depth > 0).sum())} covered pixels")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--materials", action="store_true", help="write the two material fixtures (tests/golden/pyrender_materials/) instead")
    a = ap.parse_args()
    a.out = a.out or (OUT + "_materials" if a.materials else OUT)
    try:
        import pyrender  # noqa: F401
        import trimesh  # noqa: F401
    except ImportError as e:
        sys.exit(f"{e}: this tool needs pyrender and trimesh (see the recipe in its docstring)")
    os.makedirs(a.out, exist_ok=True)
    H, W = a.height, a.width
    fx = fy = 1.1 * W
    cx, cy = W / 2 + 0.3, H / 2 - 0.2
    v, f = icosphere(3, 0.5)
    mv = np.array([[0.8, 0.0, -0.6, 0.05], [0.0, 1.0, 0.0, -0.03], [0.6, 0.0, 0.8, -2.4]])   # a rotation about y and a translation
    if a.materials:
        return materials_fixtures(a.out, mv, fx, fy, cx, cy, H, W)
    for name, vc in (("ico_plain", None), ("ico_colored", position_colors(v))):
        color, depth = render(v, f, vc, mv, fx, fy, cx, cy, H, W)
        path = os.path.join(a.out, f"{name}.npz")
        np.savez_compressed(path, vertices=v, triangles=f, vertex_colors=np.zeros((0, 4), np.uint8) if vc is None else vc, model_view=mv,
                            intrinsics=np.array([fx, fy, cx, cy]), color=color, depth=depth)
        print(f"{path}: {os.path.getsize(path)} bytes, {int((depth > 0).sum())} covered pixels, colours {np.unique(color.reshape(-1, 3), axis=0)[:4].tolist()} ...")


if __name__ == "__main__":
    main()
