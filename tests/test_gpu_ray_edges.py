"""Camera rays at the bit level, for every lens and for non-finite inputs: ``sn_camera_ray`` (signerf_amd/csrc/sn_stage.h) through the public
``Cameras.generate_rays`` paths -- ``sn_generate_rays_kernel``, ``sn_ray_batch_kernel``, ``sn_intersect_obb_kernel``.  The yardstick is
tests/ray_oracle.py: ``emulate`` (numpy fp32 in the kernel's written operand order, pinned to the CPU oracle by tests/test_ray_oracle_host.py)
and ``truth64``.  Each test prints its figures before it asserts.

A. PERSPECTIVE, no lens and each of the four DISTORTIONS: every element of origins, directions, directions_norm, pixel_area, nears and fars equals
   ``emulate`` as int32.  One thread per ray and no grid-stride loop, so small shapes: one ray, one row / one column either side of a 256-thread
   block, odd non-square frames, one 270x480, 8192-pixel strips with the principal point at the far end; two poses; pixel centres ON the
   principal point (exact-zero direction components); explicit coords, fractional and outside the image; -0.0 parameters; determinism;
   recycled output memory.
B. FISHEYE (with and without a lens) and EQUIRECTANGULAR against ``truth64``: per output |gpu - truth| <= 2 x the oracle's own maximum error on
   the case + one ulp of the element (the 2 covers device sinf / cosf against the host library's).  The fisheye principal-point ray, angles
   clipped at pi, the equirectangular poles and the +-pi seam.  nears / fars are the slab test of the GPU's OWN directions, to the bit.
C. The clamped slab test, aabb and rotated obb, every element, to the bit: a box the camera is inside, a box every ray misses, a zero-thickness
   box, an inverted box, and a box whose plane contains the camera origin under axis-parallel rays (0 / 0).
D. Non-finite and degenerate inputs (ray_oracle.nonfinite_cases: NaN / +-inf in a rotation entry and in the translation, fx = 0, fx = inf,
   fy = -0, cx = NaN, cy = inf, NaN / +-inf / +-1e30 coords, NaN / inf / +-1e30 lens parameters, NaN / +-inf box entries, NaN / inf obb T, S, R,
   zero obb S): the NaN mask of every output is the oracle's; what is not NaN equals ``emulate`` to the bit (PERSPECTIVE) or passes B's gate.
   Refused by the Python shim before any launch: an obb pose whose float64 inverse torch.linalg.inv rejects as singular -- T with an inf
   entry (``obb.T[2]=inf``) -- raises torch's linalg error.
E. ``sn_ray_batch_kernel``: one batch over all five (type, lens) branches, D's non-finite cameras and coords and the principal-point rays is
   bit-identical, NaN masks included, to the per-camera kernel, with an aabb and with an obb.

What the kernels got wrong before this file (MI355X, the parent's build): see DESIGN.md section 5 for the counts.  fminf / fmaxf drop a NaN where
the oracle's amin / amax / clamp / maximum hand it on -- in the clamped slab test (0 / 0 with the origin on a box plane and a zero direction
component; NaN or inf - inf plane distances) and in the normalisation floor (a NaN norm became 2^-50).  Both now keep it (``sn_clamped_slab``,
``sn_cam_dir``).  The fisheye angle clip also maps a NaN angle to 0, but then u or v is NaN and every output is NaN either way: no output
differs, and it is left as it was.
"""
import numpy as np
import pytest
import torch

import ray_oracle as ro
from signerf_amd import Cameras, CameraType, OrientedBox, SceneBox, scene
from test_ray_oracle_host import DISTORTIONS, LENSES, oracle_rays

pytestmark = pytest.mark.gpu

OUT = ("origins", "directions", "pixel_area", "directions_norm")
BOXED = OUT + ("nears", "fars")
T = torch.tensor


def _pose(cam=3):
    return scene.benchmark_cameras(8)[cam, :3].clone().numpy()


def _identity(origin=(0.1, 0.02, 1.0)):
    m = np.eye(4, dtype=np.float32)[:3].copy()
    m[:, 3] = origin
    return m


def _boxes(kw):
    aabb = None if kw.get("aabb") is None else SceneBox(aabb=T(ro.f32(kw["aabb"])).reshape(2, 3))
    obb = None if kw.get("obb") is None else OrientedBox(*(T(ro.f32(v)) for v in kw["obb"]))
    return aabb, obb


def _numpy(b):
    out = {"origins": b.origins, "directions": b.directions, "pixel_area": b.pixel_area, "directions_norm": b.metadata["directions_norm"]}
    if b.nears is not None:
        out["nears"], out["fars"] = b.nears, b.fars
    return {k: v.cpu().numpy() for k, v in out.items()}


def run(gpu, kw):
    """The keyword set of ro.emulate through Cameras.generate_rays -> numpy dict."""
    dist = None if kw.get("dist") is None else T(ro.f32(kw["dist"]))
    H, W = kw.get("H") or 4, kw.get("W") or 4
    cam = Cameras(T(ro.f32(kw["c2w"]))[None], kw["fx"], kw["fy"], kw["cx"], kw["cy"], W, H, distortion_params=dist,
                  camera_type=CameraType(kw.get("ctype", 1))).to(gpu)[0]
    aabb, obb = _boxes(kw)
    coords = None if kw.get("coords") is None else T(ro.f32(kw["coords"])).to(gpu)
    return _numpy(cam.generate_rays(0, coords=coords, aabb_box=aabb, obb_box=obb))


def bits(got, want, keys, label):
    """Asserts every element of every output in ``keys`` equal as int32 (NaN pattern first); prints the counts."""
    bad = {k: ro.diff_bits(got[k], want[k]) for k in keys}
    nans = {k: int(np.isnan(want[k]).sum()) for k in keys if np.isnan(want[k]).any()}
    print(f"{label}: differing elements {bad}" + (f"; NaN in the reference {nans}" if nans else ""))
    assert not any(bad.values()), (label, bad)


def _frame(H, W, pose, dist, **kw):
    f = max(H, W)
    return dict(dict(c2w=pose, fx=0.9 * f, fy=0.95 * f, cx=W / 2 + 0.25, cy=H / 2 - 0.5, H=H, W=W, dist=dist, ctype=1, aabb=ro.BOX), **kw)


# ---- A: bit parity, PERSPECTIVE ------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (257, 1), (3, 85), (37, 53), (64, 48)]
SMALL = [(1, 1), (1, 257), (257, 1), (3, 85), (37, 53)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_perspective_is_the_emulation_to_the_bit(gpu, H, W):
    for pose, tag in ((_pose(3), "camera 3"), (_identity(), "identity")):
        for i, dist in enumerate(LENSES):
            kw = _frame(H, W, pose, dist)
            bits(run(gpu, kw), ro.emulate(**kw), BOXED, f"{H}x{W} {tag} lens {i}")


@pytest.mark.parametrize("i", range(len(LENSES)))
def test_perspective_270x480_to_the_bit(gpu, i):
    kw = _frame(270, 480, _pose(0), LENSES[i])
    bits(run(gpu, kw), ro.emulate(**kw), BOXED, f"270x480 camera 0 lens {i}")


@pytest.mark.parametrize("H,W", [(1, 8192), (8192, 1)])
def test_strips_with_the_principal_point_at_the_far_end(gpu, H, W):
    """Large pixel coordinates: x - cx runs from -8000 to +192 at fx = 7373; the lens sees |u| <= 1.09."""
    for i, dist in enumerate(LENSES):
        kw = _frame(H, W, _pose(3), dist, cx=8000.25 if W > 1 else 0.75, cy=8000.25 if H > 1 else 0.25)
        bits(run(gpu, kw), ro.emulate(**kw), BOXED, f"{H}x{W} lens {i}")


@pytest.mark.parametrize("H,W,cx,cy", [(24, 40, 20.5, 11.5), (1, 257, 128.5, 0.5), (257, 1, 0.5, 200.5), (3, 85, 84.5, 2.5)])
def test_pixel_centres_on_the_principal_point(gpu, H, W, cx, cy):
    """cx = k + 0.5: with the identity rotation a column has d_x == 0 exactly and a row d_y == 0.  The origin lies on the max-x plane of the
    box, so that column's plane distance is 0 / 0: NaN nears / fars, as in the oracle."""
    for pose, tag in ((_identity((0.1, 0.02, 1.0)), "identity"), (_pose(3), "camera 3")):
        for i, dist in enumerate(LENSES):
            kw = _frame(H, W, pose, dist, cx=cx, cy=cy, fx=30.0, fy=31.0)
            e = ro.emulate(**kw)
            if tag == "identity" and dist is None:       # (a tangential lens moves the column off u == 0)
                assert int((e["directions"][..., 0] == 0).sum()) == H and int(np.isnan(e["nears"]).sum()) == H
            bits(run(gpu, kw), e, BOXED, f"{H}x{W} {tag} lens {i} principal point on a pixel centre")


@pytest.mark.parametrize("i", range(len(LENSES)))
def test_explicit_coords_fractional_and_outside(gpu, i):
    g = np.random.RandomState(11 + i)
    H, W = 37, 53
    coords = ((g.rand(3, 199, 2) * 3.0 - 1.0) * np.float32([H, W])).astype(np.float32)     # a third inside, the rest up to one image size outside
    coords[0, :5] = [[0.0, 0.0], [H, W], [-0.5, W + 0.5], [18.0, 26.75], [1e4, -1e4]]
    for pose, tag in ((_pose(3), "camera 3"), (_identity(), "identity")):
        kw = _frame(H, W, pose, LENSES[i], coords=coords)
        got = run(gpu, kw)
        assert got["directions"].shape == (3, 199, 3)
        bits(got, ro.emulate(**kw), BOXED, f"coords {tag} lens {i}")


def test_negative_zero_parameters_take_the_pinhole_path(gpu):
    kw = _frame(37, 53, _pose(3), [-0.0] * 6)
    assert not ro.has_distortion(kw["dist"])
    got = run(gpu, kw)
    bits(got, ro.emulate(**kw), BOXED, "-0.0 parameters")
    bits(got, run(gpu, dict(kw, dist=None)), BOXED, "-0.0 parameters against no parameters")
    mixed = [-0.0, 0.0, -0.0, 0.0, 1e-45, -0.0]                 # one subnormal parameter IS a lens
    kw = dict(kw, dist=mixed)
    assert ro.has_distortion(mixed)
    bits(run(gpu, kw), ro.emulate(**kw), BOXED, "one subnormal parameter")


def test_deterministic_and_on_recycled_memory(gpu):
    kw = _frame(64, 48, _pose(3), DISTORTIONS[1])
    want = ro.emulate(**kw)
    first = run(gpu, kw)
    bits(first, want, BOXED, "first run")
    # memory the allocator hands back, pre-filled: every element must be overwritten
    for sentinel in (float("nan"), -7.0e7):
        junk = [torch.full((64, 48, c), sentinel, device=gpu) for c in (3, 3, 1, 1, 1, 1)]
        torch.cuda.synchronize()
        del junk
        bits(run(gpu, kw), first, BOXED, f"after a fill with {sentinel}")


# ---- B: FISHEYE and EQUIRECTANGULAR against float64 ----------------------------------------------------------------------------------------
def accuracy(got, kw, label, nan_counts=None):
    """Part B's gate for ``got``: NaN masks are the oracle's, each of directions / norm / area within 2 x the oracle's own error + 1 ulp of
    float64 truth, origins exact, nears / fars the slab test of the GPU's own rays to the bit."""
    t, r = ro.truth64(**kw), oracle_rays(kw)
    masks = {k: (int(np.isnan(got[k]).sum()), int(np.isnan(r[k]).sum())) for k in got if not np.array_equal(np.isnan(got[k]), np.isnan(r[k]))}
    assert not masks, (label, "NaN masks (gpu, oracle)", masks)
    if nan_counts is not None:
        assert {k: int(np.isnan(got[k]).sum()) for k in OUT} == nan_counts, label
    assert ro.diff_bits(got["origins"], r["origins"]) == 0, label
    for k in ("directions", "directions_norm", "pixel_area"):
        bad, err, yard = ro.gate_failures(got[k], r[k], t[k])
        print(f"{label}: {k}: gpu error {err:.3g}, oracle's own error (yardstick) {yard:.3g}, {bad} element(s) beyond 2 x yardstick + 1 ulp")
        assert bad == 0, (label, k, err, yard)
    if "nears" in got:
        if kw.get("aabb") is not None:
            near, far = ro.slab(got["origins"], got["directions"], kw["aabb"])
        else:
            near, far = ro.slab_obb(got["origins"], got["directions"], ro.world2box(kw["obb"][0], kw["obb"][1]), kw["obb"][2])
        bad = ro.diff_bits(got["nears"].reshape(-1), near) + ro.diff_bits(got["fars"].reshape(-1), far)
        print(f"{label}: nears / fars against the slab test of the GPU's own rays: {bad} differ, {int((near < 1e10).sum())} hits")
        assert bad == 0, label


@pytest.mark.parametrize("dist", [None, DISTORTIONS[0], DISTORTIONS[1]])
@pytest.mark.parametrize("H,W", [(36, 52), (1, 257)])
def test_fisheye_against_float64(gpu, H, W, dist):
    for cam in (0, 3):
        kw = _frame(H, W, _pose(cam), dist, ctype=2)
        accuracy(run(gpu, kw), kw, f"fisheye {H}x{W} camera {cam} {'lens' if dist else 'plain'}", dict.fromkeys(OUT, 0))


@pytest.mark.parametrize("dist", [None, DISTORTIONS[0]])
def test_fisheye_principal_point_and_clipped_angles(gpu, dist):
    """cx = k + 0.5, cy = j + 0.5: the ray through the principal point is 0 / 0 -- NaN direction and norm (the oracle's torch.maximum keeps
    the NaN norm), NaN area there and at the two pixels whose +1 px neighbour it is.  fx = 4 on a 40-pixel row: angles beyond pi, clipped."""
    for pose, tag in ((_identity(), "identity"), (_pose(3), "camera 3")):
        kw = _frame(24, 40, pose, dist, ctype=2, cx=20.5, cy=11.5, fx=30.0, fy=31.0)
        accuracy(run(gpu, kw), kw, f"fisheye principal point {tag}", {"origins": 0, "directions": 3, "pixel_area": 3, "directions_norm": 1})
        kw = _frame(24, 40, pose, None, ctype=2, fx=4.0, fy=4.5)
        e = ro.emulate(**kw)
        assert (np.hypot(e["uv"][..., 0], e["uv"][..., 1]) > np.pi).sum() > 100
        accuracy(run(gpu, kw), kw, f"fisheye clipped at pi {tag}", dict.fromkeys(OUT, 0))


def test_equirectangular_against_float64_with_poles_and_seam(gpu):
    H, W = 32, 64
    for cam in (0, 4):
        kw = dict(c2w=_pose(cam), fx=float(H), fy=float(H), cx=W / 2, cy=H / 2, H=H, W=W, dist=DISTORTIONS[0], ctype=3, aabb=ro.BOX)
        accuracy(run(gpu, kw), kw, f"equirectangular {H}x{W} camera {cam}", dict.fromkeys(OUT, 0))
        # poles (v = +-1/2: y = 0, H), the seam (u = +-1: x = 0, W), both at once, and beyond both
        ys, xs = [0.0, H, H / 2, H / 4, -3.0, H + 3.0], [0.0, W, W / 2, W / 4 + 0.5, -5.0, W + 5.0]
        kw["coords"] = np.float32([[y, x] for y in ys for x in xs])
        e = ro.emulate(**kw)
        assert (np.abs(e["uv"][..., 0]) == 1).sum() == 12 and (np.abs(e["uv"][..., 1]) == 0.5).sum() == 12
        accuracy(run(gpu, kw), kw, f"equirectangular poles and seam camera {cam}", dict.fromkeys(OUT, 0))


# ---- C: slab and obb, every element ----------------------------------------------------------------------------------------------------------
ROT90 = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]     # exact in fp32, so a box plane can hold the camera origin exactly
SLAB_BOXES = {
    "camera inside": dict(aabb=[-3.0, -3.0, -3.0, 3.0, 3.0, 3.0]),
    "missed by every ray": dict(aabb=[5.0, 5.0, 5.0, 5.1, 5.1, 5.1]),
    "zero thickness": dict(aabb=[-0.12, 0.02, -0.08, 0.1, 0.02, 0.09]),
    "inverted": dict(aabb=[0.1, 0.12, 0.09, -0.12, -0.1, -0.08]),
    "plane through the origin": dict(aabb=ro.BOX),                                    # origin x = 0.1 = max x (identity pose)
    "obb: camera inside": dict(obb=(ro.OBB_R, [0.0, 0.0, 0.0], [6.0, 6.0, 6.0])),
    "obb: missed by every ray": dict(obb=(ro.OBB_R, [5.0, 5.0, 5.0], [0.1, 0.1, 0.1])),
    "obb: zero thickness": dict(obb=(ro.OBB_R, ro.OBB[1], [0.3, 0.0, 0.2])),
    "obb: inverted": dict(obb=(ro.OBB_R, ro.OBB[1], [-0.3, -0.25, -0.2])),
    "obb: hit": dict(obb=ro.OBB),
    "obb: plane through the origin": dict(obb=(ROT90, [0.0, 0.0, 0.0], [0.3, 0.2, 0.4])),  # box-frame origin y = -0.1 = -S_y / 2
}


@pytest.mark.parametrize("name", list(SLAB_BOXES))
def test_slab_every_element(gpu, name):
    box = dict(dict(aabb=None, obb=None), **SLAB_BOXES[name])
    total = 0
    for H, W in SMALL:
        for pose, tag in ((_identity(), "identity"), (_pose(3), "camera 3")):
            kw = dict(_frame(H, W, pose, None, fx=30.0, fy=31.0, cx=W // 2 + 0.5, cy=H // 2 + 0.5), **box)
            e = ro.emulate(**kw)
            total += int(np.isnan(e["nears"]).sum())
            bits(run(gpu, kw), e, BOXED, f"{name} {H}x{W} {tag}")
            kw = dict(kw, dist=DISTORTIONS[2])
            bits(run(gpu, kw), ro.emulate(**kw), ("nears", "fars"), f"{name} {H}x{W} {tag} with a lens")
    if "plane through the origin" in name:
        assert total >= 1 + 1 + 257 + 3 + 37        # the identity pose's centre column is 0 / 0 at every size
    elif name not in ("zero thickness", "inverted", "obb: zero thickness"):   # (their planes y = 0.02 and x = 0.1 hold the origin too)
        assert total == 0


def test_the_named_rays_of_the_clamped_slab(gpu):
    """Two single rays by their numbers.  Identity pose, one pixel whose centre is the principal point: d = (0, -0, -1).  From (0.1, 0, 1) --
    on the box's max-x plane -- the x distances are (-0.22 / 0, 0 / 0): NaN, NaN in the oracle (the kernel said 1e10, 1e10: a miss).  With a
    NaN in the rotation's first row d_x is NaN: NaN, NaN again (the kernel judged the ray by its other two axes: a hit)."""
    kw = dict(c2w=_identity((0.1, 0.0, 1.0)), fx=30.0, fy=31.0, cx=0.5, cy=0.5, H=1, W=1, aabb=ro.BOX)
    got = run(gpu, kw)
    assert got["directions"].reshape(3).tolist() == [0.0, 0.0, -1.0]
    r = oracle_rays(kw)
    print("origin on the max-x plane:", got["nears"].item(), got["fars"].item(), "oracle", r["nears"].item(), r["fars"].item())
    assert np.isnan(r["nears"]).all() and np.isnan(got["nears"]).all() and np.isnan(got["fars"]).all()
    c2w = _identity((0.0, 0.0, 1.0))
    c2w[0, 1] = float("nan")
    kw = dict(kw, c2w=c2w)
    got, r = run(gpu, kw), oracle_rays(kw)
    print("NaN d_x:", got["nears"].item(), got["fars"].item(), "oracle", r["nears"].item(), r["fars"].item())
    assert np.isnan(r["nears"]).all() and np.isnan(got["nears"]).all() and np.isnan(got["fars"]).all()
    # the unperturbed neighbour is a plain hit
    kw = dict(kw, c2w=_identity((0.0, 0.0, 1.0)))
    got = run(gpu, kw)
    bits(got, ro.emulate(**kw), BOXED, "the same ray from (0, 0, 1)")
    assert 0.9 < got["nears"].item() < got["fars"].item() < 1.1


# ---- D: non-finite and degenerate inputs ---------------------------------------------------------------------------------------------------
CASES = ro.nonfinite_cases(_pose(3))
GROUPS = sorted({name.split("/")[0].split("=")[0].split("[")[0] for name, _ in CASES})


@pytest.mark.parametrize("group", GROUPS)
def test_nonfinite_inputs(gpu, group):
    ran = 0
    for name, kw in CASES:
        if name.split("/")[0].split("=")[0].split("[")[0] != group:
            continue
        ran += 1
        try:
            want = ro.emulate(**kw)
        except RuntimeError:
            with pytest.raises(RuntimeError, match="singular"):      # the shim's float64 inverse refuses the pose before any launch
                run(gpu, kw)
            print(f"{name}: refused")
            continue
        got, r = run(gpu, kw), oracle_rays(kw)
        masks = {k: (int(np.isnan(got[k]).sum()), int(np.isnan(r[k]).sum())) for k in BOXED if not np.array_equal(np.isnan(got[k]), np.isnan(r[k]))}
        assert not masks, (name, "NaN masks (gpu, oracle)", masks)
        if kw["ctype"] == 1:
            bits(got, want, BOXED, name)
        else:
            accuracy(got, kw, name)
    assert ran > 0


# ---- E: the ray batch kernel does the same arithmetic ------------------------------------------------------------------------------------------
def _batch_cameras():
    """One Cameras batch: the five (type, lens) branches, every camera-side case of part D (pose, intrinsics, lens parameters), the
    principal-point cameras (identity pose, cx = 3.5, cy = 2.5)."""
    rows = []
    for ct, dist in ((1, None), (1, ro.LENS), (2, None), (2, ro.LENS), (3, None), (3, ro.LENS)):
        rows.append(dict(c2w=_pose(3), fx=6.5, fy=6.25, cx=3.5, cy=2.25, dist=dist, ctype=ct))
        rows.append(dict(c2w=_identity(), fx=6.5, fy=6.25, cx=3.5, cy=2.5, dist=dist, ctype=ct))
    seen = set()
    for name, kw in CASES:
        if kw["coords"] is not None or kw["obb"] is not None or kw["aabb"] != ro.BOX:
            continue
        row = dict(c2w=kw["c2w"], fx=kw["fx"], fy=kw["fy"], cx=kw["cx"], cy=kw["cy"], dist=kw["dist"], ctype=kw["ctype"])
        key = repr([(k, np.asarray(v if v is not None else [0.0] * 6, dtype=np.float32).tobytes()) for k, v in row.items()])
        if key not in seen:
            seen.add(key)
            rows.append(row)
    return rows


@pytest.mark.parametrize("box", ["aabb", "obb", "aabb with a NaN entry", "none"])
def test_ray_batch_is_the_per_camera_kernel_to_the_bit(gpu, box):
    rows = _batch_cameras()
    B = len(rows)
    dist = torch.stack([T(ro.f32(r["dist"] if r["dist"] is not None else [0.0] * 6)) for r in rows])
    col = lambda k: T([float(r[k]) for r in rows], dtype=torch.float32)[:, None]  # noqa: E731
    cams = Cameras(torch.stack([T(ro.f32(r["c2w"])) for r in rows]), col("fx"), col("fy"), col("cx"), col("cy"), 7, 5, distortion_params=dist,
                   camera_type=[r["ctype"] for r in rows]).to(gpu)
    nan, inf = float("nan"), float("inf")
    ys, xs = np.divmod(np.arange(35), 7)
    coords = np.concatenate([np.stack([ys + 0.5, xs + 0.5], -1).astype(np.float32),
                             np.float32([[nan, 1.5], [2.5, nan], [inf, 1.0], [1.0, -inf], [1e30, 2.0], [3.0, 1e30], [-1e30, -1e30], [nan, nan],
                                         [2.25, 3.5], [1.75, 6.125], [-4.0, 9.5]])])
    n = coords.shape[0]
    # every camera sees every coordinate, interleaved so that neighbouring lanes take different branches
    ci = torch.arange(B).repeat(n)
    cc = T(coords).repeat_interleave(B, dim=0)
    kw = {"aabb": dict(aabb=ro.BOX), "obb": dict(obb=ro.OBB), "aabb with a NaN entry": dict(aabb=[-0.12, nan, -0.08, 0.1, 0.12, 0.09]), "none": {}}[box]
    aabb, obb = _boxes(kw)
    keys = BOXED if kw else OUT
    batch = _numpy(cams.generate_rays(camera_indices=ci.to(gpu)[:, None], coords=cc.to(gpu), aabb_box=aabb, obb_box=obb))
    assert batch["directions"].shape == (B * n, 3) and (("nears" in batch) == bool(kw))
    bad = dict.fromkeys(keys, 0)
    nans = dict.fromkeys(keys, 0)
    for c in range(B):
        one = _numpy(cams[c].generate_rays(0, coords=T(coords).to(gpu), aabb_box=aabb, obb_box=obb))
        for k in keys:
            bad[k] += ro.diff_bits(batch[k][c::B], one[k])
            nans[k] += int(np.isnan(one[k]).sum())
    print(f"{B} cameras x {n} coords, {box}: differing elements {bad}; NaN elements {nans}")
    assert not any(bad.values()), bad
    assert nans["directions"] > 0 and nans["directions"] < 3 * B * n
    # and the per-camera kernel is the emulation's for the PERSPECTIVE cameras of the batch (so both are)
    for c in [i for i, r in enumerate(rows) if r["ctype"] == 1][:6]:
        r = rows[c]
        e = ro.emulate(r["c2w"], r["fx"], r["fy"], r["cx"], r["cy"], dist=r["dist"], coords=coords, **kw)
        bits({k: batch[k][c::B] for k in keys}, e, keys, f"batch camera {c} against the emulation")
