"""Lens-aware proxy mesh, CPU side: the ``lens`` field, the companion C header include/signerf_hip_mesh_rays.h against the binding and the
library's exports, its argument checks, the host BVH builder, known answers of the float64 ray-cast oracle (tests/mesh_rays_oracle.py) and
the choice of the oracle's eps.  No GPU.

How eps was chosen (``test_eps_separates_fp32_from_fp64`` re-runs it on reduced views; the full run is
``python tests/test_mesh_rays_host.py``).  The oracle was run twice on every view of ``mesh_rays_oracle.views()`` -- float64 and a float32
copy of itself -- from the same fp32 rays.  The two disagree (coverage or hit triangle) on DISAGREE rays; the smallest eps whose flags
hide all of them is EPS_NEEDED, the largest edge distance among them.  FLAGGED: the share of the pixels / of the covered pixels with an
edge distance below 1e-4, eight times EPS (the shares at EPS itself are smaller):

    view                 pixels   covered  disagree  eps_needed  flagged at 1e-4, of pixels / of covered
    pinhole_0_800        640000   0.4567   0         0           0.00028 / 0.00061
    pinhole_3_800        640000   0.4781   0         0           0.00029 / 0.00061
    pinhole_5_800        640000   0.4608   2         2.99e-06    0.00025 / 0.00055
    pinhole_1_531x397    210807   0.5913   0         0           0.00035 / 0.00059
    opencv_2_640x480     307200   0.3648   0         0           0.00022 / 0.00061
    fisheye_4_512        262144   0.1019   0         0           0.00010 / 0.00097
    equirect_512x256     131072   0.0681   0         0           0 / 0   (its camera was first 0.24 from the mesh: 0.038 covered, too little)

EPS = 4 x max(eps_needed) = 4 x 2.99e-06 = 1.2e-5.  Caps: 0.005 of the pixels, 0.05 of the covered pixels; every view is more than ten
times inside both, and the mesh covers at least 0.068 of each view (0.05 asked).  At EPS itself, from the rays the GPU generates
(printed by the GPU tests): 5, 3 and 0 flagged rays on the OPENCV, FISHEYE and EQUIRECTANGULAR views.

For the comparison with the RASTERISER (test 1 of tests/test_gpu_mesh_rays.py) the same procedure was run between tests/mesh_oracle.py
(the float64 restatement of the raster's screen-space edge rule) and the ray-cast oracle on the four pinhole views: they do not disagree
in coverage on a single pixel (eps needed 0), so no second eps is needed.  That test also excuses the pixels mesh_oracle itself marks
ambiguous -- its own eps = 1e-5 of normalised edge distance, the rule the raster kernel is tested with in tests/test_gpu_mesh_raster.py --
and counts them towards the caps: with them 0.0017-0.0024 of the pixels and 0.0036-0.0040 of the covered ones are flagged, nearly all
by that rule.

Depth tolerance Z_RTOL: 4 x the larger of the two kernels' own errors against the float64 oracle on the
unflagged pixels of the pinhole views.  Measured on an MI355X (relative, maximum over the unflagged covered pixels): ray cast 1.22e-05 /
6.6e-06 / 1.39e-05 / 5.7e-06, raster 8.7e-06 / 1.18e-05 / 9.7e-06 / 5.9e-06 on the four views, so Z_RTOL = 4 x 1.39e-05 = 5.6e-5.
These errors are the conditioning of the depth of a grazing triangle, not the kernels' arithmetic: the float32 copy of the oracle is
7.9e-06 / 6.1e-06 / 1.6e-05 / 2.4e-05 from the float64 one on the same views, and the two float64 oracles (raster and ray cast), which
differ only by the fp32 rounding of the rays, are 6.7e-06 / 7.4e-06 / 9.2e-06 / 4.9e-06 apart.
"""
import ctypes as C

import numpy as np
import pytest

import mesh_oracle as mo
import mesh_rays_oracle as mro
from abi_helpers import c99_probe, refusal_sweep
from signerf_amd import _lib
from signerf_amd.renderer import ACCEL_LEAF_MAX, Renderer, RendererConfig, build_accel, object_pose

EPS, Z_RTOL = mro.EPS, mro.Z_RTOL


# ---- the config field ------------------------------------------------------------------------------------------------------------------
def test_lens_field_default_and_validation():
    assert RendererConfig().lens == "pinhole"
    assert Renderer(RendererConfig(lens="camera"), device="cpu").config.lens == "camera"
    with pytest.raises(ValueError, match="lens"):
        Renderer(RendererConfig(lens="nonsense"), device="cpu")


def test_lens_is_recorded_in_config_yml(tmp_path):
    import yaml

    from signerf_amd.datasetgenerator import DatasetGenerator, DatasetGeneratorConfig

    cfg = DatasetGeneratorConfig(path=tmp_path, dataset_name="s", width=8, height=8, masking_mode="shape",
                                 renderer=RendererConfig(object_path="proxy.obj", lens="camera"))
    g = DatasetGenerator(cfg, device="cpu", write_images=False)
    g.init_directory()
    assert yaml.safe_load((tmp_path / "s" / "config.yml").read_text())["renderer"]["lens"] == "camera"
    g.dataset.close()
    with pytest.raises(ValueError, match="lens"):
        DatasetGenerator(DatasetGeneratorConfig(path=tmp_path, dataset_name="t", masking_mode="shape", renderer=RendererConfig(lens="wide")), device="cpu")


def test_setup_builds_the_accel_only_for_the_camera_lens(tmp_path):
    v, f = mo.icosphere(1)
    with open(tmp_path / "m.obj", "w") as fh:
        fh.write("".join(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in v.tolist()) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.tolist()))
    r = Renderer(RendererConfig(object_path=str(tmp_path / "m.obj")), device="cpu")
    r.setup()
    assert r._host_accel is None
    r = Renderer(RendererConfig(object_path=str(tmp_path / "m.obj"), lens="camera", position=[0.1, 0.0, 0.0]), device="cpu")
    assert r._host_accel is None   # before setup()
    from signerf_amd import Cameras, scene

    with pytest.raises(RuntimeError, match="setup"):
        r.render_camera(Cameras(scene.benchmark_cameras(8)[:, :3], 10.0, 10.0, 4.0, 4.0, 8, 8)[0])
    r.setup()
    nodes, recs, n_nodes = _parse(r._host_accel, f.shape[0])
    world = mro.posed(v, object_pose(r.config))
    np.testing.assert_array_equal(recs["corners"][np.argsort(recs["index"])], world[f])   # the POSED corners


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
def test_mesh_rays_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    lib = _lib.load()
    assert lib.sn_mesh_rays_abi_version() == _lib.header("mesh_rays").version == 1
    assert lib.sn_mesh_abi_version() == 1 and lib.sn_mesh_color_abi_version() == 1   # the two raster headers are untouched
    assert b"sn_mesh_rays_kernel" in open(built_lib, "rb").read()


def test_rays_opts_layout_matches_c(tmp_path):
    got = [int(x) for x in c99_probe(tmp_path, "signerf_hip_mesh_rays.h", "%zu %zu %zu %zu %zu %d",
                                     "sizeof(SnMeshRaysOpts), offsetof(SnMeshRaysOpts, struct_size), offsetof(SnMeshRaysOpts, znear), "
                                     "offsetof(SnMeshRaysOpts, zfar), offsetof(SnMeshRaysOpts, cull_back_faces), SN_MESH_RAYS_ABI_VERSION")]
    o = _lib.SnMeshRaysOpts
    assert got == [C.sizeof(o), o.struct_size.offset, o.znear.offset, o.zfar.offset, o.cull_back_faces.offset,
                   _lib.header("mesh_rays").version]
    assert _lib.SnMeshRaysOpts().struct_size == C.sizeof(o)


_NULL_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
fake = 0x1000   # never dereferenced: every call below is refused before the device is touched
fwd = (C.c_float * 3)(0, 0, -1)
F = 10
nb = lib.sn_mesh_accel_bytes(F)
def opts(size=None, znear=1e-4, zfar=10.0):
    o = _lib.SnMeshRaysOpts(); o.znear, o.zfar = znear, zfar
    if size is not None: o.struct_size = size
    return C.byref(o)
def sopts(size=None, nan=False):
    o = _lib.SnMeshShadeOpts(); o.base_color[:] = [0.3, 0.3, 0.3, 1.0]; o.ambient[:] = [1.0, 1.0, 1.0]; o.background[:] = [1.0, 1.0, 1.0]
    if nan: o.ambient[1] = float("nan")
    if size is not None: o.struct_size = size
    return C.byref(o)
def cast(o=fake, d=fake, h=4, w=4, f=fwd, accel=fake, nbytes=nb, tris=fake, op=None, shade=None, depth=fake, color=N):
    return lib.sn_mesh_cast_rays(o, d, h, w, f, accel, nbytes, tris, F, N, 30, op if op is not None else opts(), shade, depth, color, N)
calls = {
 "abi": lambda: lib.sn_mesh_rays_abi_version(),
 "accel_bytes_negative": lambda: lib.sn_mesh_accel_bytes(-1),
 "accel_bytes_too_many": lambda: lib.sn_mesh_accel_bytes((1 << 26) + 1),
 "all_null": lambda: lib.sn_mesh_cast_rays(N, N, 4, 4, None, N, 0, N, F, N, 0, None, None, N, N, N),
 "no_origins": lambda: cast(o=N),
 "no_directions": lambda: cast(d=N),
 "no_forward": lambda: cast(f=None),
 "zero_forward": lambda: cast(f=(C.c_float * 3)(0, 0, 0)),
 "null_accel": lambda: cast(accel=N),
 "accel_wrong_size": lambda: cast(nbytes=nb - 16),
 "accel_misaligned": lambda: cast(accel=fake + 4),
 "no_depth": lambda: cast(depth=N),
 "height_0": lambda: cast(h=0),
 "width_big": lambda: cast(w=16385),
 "opts_size0": lambda: cast(op=opts(0)),
 "opts_newer": lambda: cast(op=opts(64)),
 "znear_0": lambda: cast(op=opts(znear=0.0)),
 "zfar_below_znear": lambda: cast(op=opts(znear=1.0, zfar=0.5)),
 "color_without_shade": lambda: cast(color=fake),
 "color_without_triangles": lambda: cast(color=fake, shade=sopts(), tris=N),
 "color_shade_size0": lambda: cast(color=fake, shade=sopts(0)),
 "color_shade_nan": lambda: cast(color=fake, shade=sopts(nan=True)),
}
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_cast_rays_refuses_bad_arguments_before_the_device(built_lib):
    """NULL pointers (the accel blob among them), a struct_size of 0 or of a newer layout, bad planes / sizes / blob sizes: refused with
    SN_ERR_INVALID (size queries: 0) in a child process -- nothing is launched, and a crash would be a segfault, not an exception."""
    got = refusal_sweep(_NULL_SWEEP)
    want = {k: "1" for k in got}
    want.update({"abi": "1", "accel_bytes_negative": "0", "accel_bytes_too_many": "0"})
    assert len(got) == 22 and got == want


# ---- the host BVH builder --------------------------------------------------------------------------------------------------------------
def _parse(blob, F):
    """The blob as csrc/sn_mesh_rays.h lays it out -> (nodes: structured [n_nodes], triangle records: structured [F], n_nodes)."""
    assert blob.dtype == np.uint8 and blob.ndim == 1
    head = blob[:64].view(np.uint32)
    assert head[0] == 0x31524D53 and head[1] == 1 and head[2] == F and (head[4:] == 0).all()
    n_nodes, cap = int(head[3]), max(F, 1)
    assert 1 <= n_nodes <= cap and blob.size == 64 + 64 * cap + 48 * F
    node_t = np.dtype([("lmin", "<f4", 3), ("lmax", "<f4", 3), ("rmin", "<f4", 3), ("rmax", "<f4", 3), ("child", "<i4", 2), ("pad", "<i4", 2)])
    tri_t = np.dtype([("corners", "<f4", (3, 3)), ("index", "<i4"), ("pad", "<i4", 2)])
    nodes = blob[64:64 + 64 * cap].view(node_t)
    return nodes[:n_nodes], blob[64 + 64 * cap:].view(tri_t), n_nodes


def _check_tree(blob, world, tris):
    """Every triangle in exactly one leaf, every box bounds everything below it, every inner node reached once, depth <= 32."""
    F = tris.shape[0]
    nodes, recs, n_nodes = _parse(blob, F)
    assert sorted(recs["index"].tolist()) == list(range(F))
    np.testing.assert_array_equal(recs["corners"], world[tris][recs["index"]])
    seen_tri, seen_node, max_depth = np.zeros(F, dtype=int), np.zeros(n_nodes, dtype=int), 0

    def below(child, depth):
        """(lo, hi) of the triangles under `child`, visiting them."""
        nonlocal max_depth
        max_depth = max(max_depth, depth)
        if child < 0:
            ref = -(child + 1)
            first, count = ref >> 3, ref & 7
            assert count <= ACCEL_LEAF_MAX and first + count <= F
            seen_tri[first:first + count] += 1
            c = recs["corners"][first:first + count].reshape(-1, 3)
            return (c.min(0), c.max(0)) if count else (np.full(3, np.inf), np.full(3, -np.inf))
        seen_node[child] += 1
        nd = nodes[child]
        los, his = [], []
        for side, (bmin, bmax) in enumerate(((nd["lmin"], nd["lmax"]), (nd["rmin"], nd["rmax"]))):
            lo, hi = below(int(nd["child"][side]), depth + 1)
            assert (bmin <= lo).all() and (bmax >= hi).all(), (child, side)
            los.append(lo)
            his.append(hi)
        return np.minimum(*los), np.maximum(*his)

    below(0, 0)
    assert (seen_tri == 1).all() and (seen_node == 1).all() and max_depth <= 32
    return n_nodes, max_depth


def test_bvh_of_the_bunny_stand_in(built_lib):
    v, f, _ = mro.bumpy_sphere()
    world = mro.posed(v, object_pose(RendererConfig(scale=mro.BUNNY_SCALE)))
    blob = build_accel(world, f)
    assert blob.size == _lib.load().sn_mesh_accel_bytes(f.shape[0])
    n_nodes, depth = _check_tree(blob, world, f)
    assert depth <= 13 and n_nodes < f.shape[0] // 2   # a median split of 5 120 triangles into leaves of <= 4: 11 levels


def test_bvh_of_degenerate_and_tiny_meshes(built_lib):
    lib = _lib.load()
    # coincident vertices: 40 triangles that are all the same point, 30 that share one edge, a few ordinary ones
    v = np.zeros((12, 3), np.float32)
    v[1], v[2], v[3:] = [1, 0, 0], [1, 0, 0], np.random.default_rng(0).uniform(-1, 1, (9, 3))
    f = np.array([[0, 0, 0]] * 40 + [[1, 2, 1]] * 30 + [[3, 4, 5], [6, 7, 8], [9, 10, 11], [0, 1, 3]], np.int32)
    blob = build_accel(v, f)
    assert blob.size == lib.sn_mesh_accel_bytes(f.shape[0])
    _check_tree(blob, v, f)
    for n in (0, 1, 4, 5, 9):   # no triangle, one leaf, the first split
        v, f = mo.triangle_soup(n, seed=n)
        blob = build_accel(v, f)
        assert blob.size == lib.sn_mesh_accel_bytes(n)
        _check_tree(blob, v, f)
    # an index outside the vertices, a non-finite corner: kept (every triangle once), with all corners at the origin
    v, f = mo.triangle_soup(6, seed=1)
    f = f.copy()
    f[2, 1] = 99
    v[f[4, 0]] = np.nan
    nodes, recs, _ = _parse(build_accel(v, f), 6)
    by_index = recs["corners"][np.argsort(recs["index"])]
    assert (by_index[2] == 0).all() and (by_index[4] == 0).all() and np.isfinite(recs["corners"]).all()
    np.testing.assert_array_equal(by_index[0], v[f[0]])


def _walk(blob, F, o, d, fwd, znear=1e-4, zfar=10.0, cull=True):
    """The kernel's traversal (csrc/sn_mesh_rays.h) for one ray, in fp32 scalars -> (z, triangle)."""
    f32 = np.float32
    nodes, recs, n_nodes = _parse(blob, F)
    o, d = o.astype(f32), d.astype(f32)
    f = f32(d @ fwd.astype(f32))
    best, tri = f32(np.inf), -1
    if not f > 0:
        return 0.0, -1
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = np.where(np.abs(d) >= 1e-20, f32(1) / d, np.copysign(f32(1e20), d)).astype(f32)

        def box(lo, hi):
            t0, t1 = (lo - o) * inv, (hi - o) * inv
            tn = max(f32(0), np.fmin(t0, t1).max())
            tf = min(best, (np.fmax(t0, t1) * f32(1.0000005)).min())
            return tn if tn <= tf else f32(np.inf)

        def leaf(child):
            nonlocal best, tri
            ref = -(child + 1)
            for k in range(ref >> 3, (ref >> 3) + (ref & 7)):
                a, b, c = recs["corners"][k]
                e1, e2, tv = b - a, c - a, o - a
                pv = np.cross(d, e2).astype(f32)
                det = f32(e1 @ pv)
                if (cull and not det > 0) or det == 0:
                    continue
                u = f32(tv @ pv) / det
                qv = np.cross(tv, e1).astype(f32)
                v, t = f32(d @ qv) / det, f32(e2 @ qv) / det
                z = t * f
                if u >= 0 and v >= 0 and u + v <= 1 and t > 0 and znear < z < zfar and (t < best or (t == best and recs["index"][k] < tri)):
                    best, tri = t, int(recs["index"][k])

        stack, node = [], 0
        for _ in range(2 * n_nodes):
            nd = nodes[node]
            cl, cr = int(nd["child"][0]), int(nd["child"][1])
            tl = box(nd["lmin"], nd["lmax"])
            if cl < 0:
                if np.isfinite(tl):
                    leaf(cl)
                tl = f32(np.inf)
            tr = box(nd["rmin"], nd["rmax"])
            if cr < 0:
                if np.isfinite(tr):
                    leaf(cr)
                tr = f32(np.inf)
            if np.isfinite(tl) and np.isfinite(tr):
                stack.append(cl if tr < tl else cr)
                node = cr if tr < tl else cl
            elif np.isfinite(tl):
                node = cl
            elif np.isfinite(tr):
                node = cr
            elif stack:
                node = stack.pop()
            else:
                break
    return (float(best * f), tri) if tri >= 0 else (0.0, -1)


def test_walking_the_blob_finds_the_oracles_hits():
    """A restatement of the kernel's traversal over the builder's blob, ray by ray in fp32, against the brute-force float64 oracle: the
    hierarchy loses no hit (every 97th ray of a 96 x 96 view of the bunny stand-in and of the rays that graze its outline)."""
    v, f, _ = mro.bumpy_sphere()
    world = mro.posed(v, object_pose(RendererConfig(scale=mro.BUNNY_SCALE)))
    blob = build_accel(world, f)
    view = dict(mro.views()["pinhole_3_800"], fx=115.0, fy=115.0, cx=48.0, cy=48.0, W=96, H=96)
    o, d = mro.cpu_rays(view)
    fwd = mro.forward_of(view["c2w"])
    z, tri, edge, _ = mro.cast(o, d, fwd, world, f)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    cov = z > 0
    assert 0.3 < cov.mean() < 0.6
    picks = sorted(set(range(0, z.size, 97)) | set(np.nonzero(edge < 0.05)[0][::23].tolist()))
    checked = 0
    for i in picks:
        if edge[i] < EPS:
            continue
        zz, tt = _walk(blob, f.shape[0], o[i], d[i], fwd)
        assert (zz > 0) == cov[i] and tt == tri[i], i
        if cov[i]:
            assert abs(zz - z[i]) <= Z_RTOL * z[i]
        checked += 1
    assert checked > 100


# ---- known answers of the oracle ---------------------------------------------------------------------------------------------------------
def _one_triangle(dist, flip=False):
    """A triangle facing a camera at the origin that looks down -z, at distance `dist`."""
    v = np.array([[-0.5, -0.4, -dist], [0.6, -0.3, -dist], [0.0, 0.7, -dist]], np.float32)
    return v, np.array([[0, 2, 1] if flip else [0, 1, 2]], np.int32)


def _pinhole_rays(H=33, W=33, F=30.0):
    view = dict(c2w=np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32), fx=F, fy=F, cx=W / 2, cy=H / 2, W=W, H=H, distortion=None,
                camera_type=mro.PERSPECTIVE)
    return mro.cpu_rays(view)


def test_oracle_single_triangle_known_answers():
    o, d = _pinhole_rays()
    fwd = np.array([0.0, 0.0, -1.0])
    v, f = _one_triangle(2.5)
    z, tri, edge, ff = mro.cast(o, d, fwd, v, f)
    z, tri = z.reshape(33, 33), tri.reshape(33, 33)
    assert abs(z[16, 16] - 2.5) < 1e-6 and tri[16, 16] == 0   # the centre pixel looks down the axis: z = d
    cov = z > 0
    np.testing.assert_allclose(z[cov], 2.5, rtol=1e-6)          # z-depth, not ray length: the triangle is parallel to the image plane
    # its outline: the projection of the three corners; outside it nothing is drawn
    j, i = np.meshgrid(np.arange(33) + 0.5, np.arange(33) + 0.5)
    x, y = (j - 16.5) / 30.0 * 2.5, -(i - 16.5) / 30.0 * 2.5
    a, b, c = v[:, :2].astype(np.float64)
    e = lambda p, q: (q[0] - p[0]) * (y - p[1]) - (q[1] - p[1]) * (x - p[0])  # noqa: E731
    inside = (e(a, b) > 0) & (e(b, c) > 0) & (e(c, a) > 0)
    sure = np.minimum(np.minimum(np.abs(e(a, b)), np.abs(e(b, c))), np.abs(e(c, a))) > 1e-6
    assert (cov == inside)[sure].all() and inside.sum() > 50 and (~inside).sum() > 50
    assert (edge.reshape(33, 33)[~cov & sure] > 0).all()
    # the winding: culled when clockwise, drawn again without culling
    vz, fz = _one_triangle(2.5, flip=True)
    assert not (mro.cast(o, d, fwd, vz, fz)[0] > 0).any()
    np.testing.assert_array_equal(mro.cast(o, d, fwd, vz, fz, cull=False)[0] > 0, cov.reshape(-1))
    # beyond zfar, before znear, behind the camera
    assert not (mro.cast(o, d, fwd, *_one_triangle(12.0))[0] > 0).any()
    assert (mro.cast(o, d, fwd, *_one_triangle(12.0), zfar=20.0)[0] > 0).any()
    assert not (mro.cast(o, d, fwd, *_one_triangle(2.5), znear=3.0)[0] > 0).any()
    behind = (v * np.array([1, 1, -1], np.float32), f)
    assert not (mro.cast(o, d, fwd, *behind, cull=False)[0] > 0).any()
    # rays that point backwards draw nothing even where they hit: the same scene seen with the viewing axis reversed
    zb, _, _, fb = mro.cast(o, d, -fwd, v, f, cull=False)
    assert (fb < 0).all() and not (zb > 0).any()


def test_oracle_nearest_hit_and_undrawn_hits_do_not_occlude():
    o, d = _pinhole_rays()
    fwd = np.array([0.0, 0.0, -1.0])
    near, far = _one_triangle(1.0), _one_triangle(2.0)
    v = np.concatenate([far[0], near[0]])
    f = np.concatenate([far[1], near[1] + 3])
    z, tri, _, _ = mro.cast(o, d, fwd, v, f)
    assert tri[16 * 33 + 16] == 1 and abs(z[16 * 33 + 16] - 1.0) < 1e-6
    # the near one culled (clockwise) or before znear: the far one shows through, as the rasteriser clips and culls before its depth test
    f2 = f.copy()
    f2[1] = f2[1][[0, 2, 1]]
    assert mro.cast(o, d, fwd, v, f2)[1][16 * 33 + 16] == 0
    assert mro.cast(o, d, fwd, v, f, znear=1.5)[1][16 * 33 + 16] == 0


def test_oracle_agrees_with_the_raster_oracle_on_a_pinhole():
    """The ray-cast oracle and the float64 restatement of the rasteriser (tests/mesh_oracle.py) draw the same picture through a pinhole."""
    from signerf_amd.renderer import model_view

    v, f, _ = mro.bumpy_sphere(2)
    pose = object_pose(RendererConfig(scale=mro.BUNNY_SCALE, rotation=[10, 20, 30]))
    view = dict(mro.views()["pinhole_0_800"], fx=150.0, fy=150.0, cx=64.0, cy=60.0, W=128, H=120)
    o, d = mro.cpu_rays(view)
    z, tri, edge, _ = mro.cast(o, d, mro.forward_of(view["c2w"]), mro.posed(v, pose), f)
    ref, amb, _ = mo.raster_depth(v, f, model_view(view["c2w"].reshape(-1).tolist(), pose), 150.0, 150.0, 64.0, 60.0, 120, 128)
    ref, ok = ref.reshape(-1), ~amb.reshape(-1) & ~(edge < EPS)
    assert ((ref > 0) == (z > 0))[ok].all() and (z > 0).mean() > 0.2
    both = ok & (z > 0)
    assert (np.abs(ref - z)[both] <= 1e-6 * z[both]).all()


# ---- eps -------------------------------------------------------------------------------------------------------------------------------
def _fp32_vs_fp64(view, world, f):
    o, d = mro.cpu_rays(view)
    fwd = mro.forward_of(view["c2w"])
    z64, t64, e64, ff = mro.cast(o, d, fwd, world, f)
    z32, t32, _, _ = mro.cast(o, d, fwd, world, f, dtype=np.float32)
    cov = z64 > 0
    dis = ((z32 > 0) != cov) | ((t32 != t64) & cov)
    ok = cov & (z32 > 0) & ~(e64 < EPS)
    return dict(pixels=cov.size, covered=float(cov.mean()), disagree=int(dis.sum()), eps_needed=float(e64[dis].max()) if dis.any() else 0.0,
                shares=mro.flagged_shares(e64 < EPS, cov), z_err=float((np.abs(z32 - z64)[ok] / z64[ok]).max()), backwards=int((ff <= 0).sum()))


@pytest.mark.parametrize("name", ["opencv_2_640x480", "equirect_512x256"])
def test_eps_separates_fp32_from_fp64(name):
    """The procedure of the module docstring on two of the views at a quarter of their size (the full sizes: run this file as a script):
    the float32 copy of the oracle disagrees with the float64 one only on rays flagged at EPS / 4, the flags stay inside the caps, the
    mesh covers at least 5 % of the view, and off the flags the fp32 depth is inside Z_RTOL."""
    v, f, _ = mro.bumpy_sphere()
    world = mro.posed(v, object_pose(RendererConfig(scale=mro.BUNNY_SCALE)))
    view = dict(mro.views()[name])
    for k in ("fx", "fy", "cx", "cy"):
        view[k] = view[k] / 4
    view["W"], view["H"] = view["W"] // 4, view["H"] // 4
    r = _fp32_vs_fp64(view, world, f)
    assert r["eps_needed"] <= EPS / 4, r
    assert r["shares"][0] <= mro.MAX_FLAGGED_OF_PIXELS and r["shares"][1] <= mro.MAX_FLAGGED_OF_COVERED and r["covered"] >= 0.05, r
    assert r["z_err"] <= Z_RTOL, r
    if name.startswith("equirect"):
        assert r["backwards"] > 0.4 * r["pixels"]   # half of the sphere of directions points backwards


if __name__ == "__main__":   # the figures of the module docstring
    v_, f_, _ = mro.bumpy_sphere()
    world_ = mro.posed(v_, object_pose(RendererConfig(scale=mro.BUNNY_SCALE)))
    for name_, view_ in mro.views().items():
        print(name_, _fp32_vs_fp64(view_, world_, f_), flush=True)
