"""Pins tests/ray_oracle.py::emulate -- the numpy fp32 restatement of ``sn_camera_ray`` that tests/test_gpu_ray_edges.py holds the kernels to, bit for
bit -- against the CPU oracle (oracle/nerfacto.py), without a GPU.  All four lenses of tests/test_gpu_cameras.py::DISTORTIONS, the three camera
types, cameras 0 and 3 of ``scene.benchmark_cameras(8)`` with that file's intrinsics.  Every test prints its figures before it asserts.

What is bit-equal to the oracle: the un-distorted image-plane points (10 Newton steps), the origins, and the clamped slab tests given the same
rays -- every NaN included.  What cannot be: ``torch.linalg.vector_norm`` accumulates the three squares differently from the kernel's written
``(a*a + b*b) + c*c``, so the norm differs by one ulp in a few per cent of the pixels and the directions by one rounding of the quotient:

    PERSPECTIVE, 270x480, camera 3 (measured here): directions differ in 7.2-7.6 % of the elements, by <= 1.19e-7; directions_norm in
    7.2-7.8 % of the pixels; pixel_area by <= 4.7e-5 relative, 3.8e-4 for the degenerate lens (no lens, DISTORTIONS[0], DISTORTIONS[3]).

For PERSPECTIVE the directions are gated at 1.2e-7 absolute (one ulp of an element in [0.5, 1)).  FISHEYE / EQUIRECTANGULAR additionally go through
sin / cos, where numpy (libm) and torch (its vectorised library) differ by an ulp in 7-12 % of the angles, and torch's ``sqrt(sum(c**2))`` is not the
written ``sqrt(u*u + v*v)`` to the bit either; the directions then differ in 9-29 % of the elements, by up to 1.3e-7 (3.3e-7 for DISTORTIONS[3],
whose Newton iteration diverges in part of the frame): the 1.2e-7 of the PERSPECTIVE cases is one norm ulp and does not cover a second library.
Those lenses are not compared bit for bit anywhere; their figure is printed and their gate is the accuracy one below.

Accuracy: emulation and oracle against ``truth64`` (the same geometry in float64 from the same fp32 inputs); per output and per case the
emulation's maximum error must not exceed twice the oracle's own.  The factor of 2 is the one-ulp norm difference.
"""
import numpy as np
import pytest
import torch

import ray_oracle as ro
from oracle import nerfacto as onf
from signerf_amd import scene

DISTORTIONS = [
    [0.05, -0.02, 0.0, 0.0, 0.001, -0.002],
    [-0.28, 0.09, -0.01, 0.002, 0.0, 0.0],
    [0.0, 0.0, 0.0, 0.0, 0.01, 0.02],
    [-1.5, 0.3, 0.0, 0.0, 0.05, 0.0],
]
LENSES = [None] + DISTORTIONS
CAMERAS = (0, 3)
OUTPUTS = ("origins", "directions", "pixel_area", "directions_norm")
T = torch.tensor


def _intrinsics(H, W):
    return 0.9 * W, 0.95 * W, W / 2 + 0.25, H / 2 - 0.5     # tests/test_gpu_cameras.py::_cam


def _c2w(cam):
    return scene.benchmark_cameras(8)[cam, :3].clone()


def oracle_rays(kw):
    """onf.generate_rays (+ intersect_aabb_ns / intersect_obb on the oracle's own rays) for the keyword set of ro.emulate -> numpy dict."""
    r = onf.generate_rays(T(ro.f32(kw["c2w"])), kw["fx"], kw["fy"], kw["cx"], kw["cy"], kw.get("H"), kw.get("W"),
                          None if kw.get("dist") is None else T(kw["dist"]), kw.get("ctype", 1),
                          None if kw.get("coords") is None else T(ro.f32(kw["coords"])))
    out = {k: r[k].numpy() for k in OUTPUTS}
    o, d = r["origins"].reshape(-1, 3), r["directions"].reshape(-1, 3)
    if kw.get("aabb") is not None:
        n, f = onf.intersect_aabb_ns(o, d, T(ro.f32(kw["aabb"])).reshape(6))
    elif kw.get("obb") is not None:
        n, f = onf.intersect_obb(o, d, *(T(ro.f32(v)) for v in kw["obb"]))
    else:
        return out
    out["nears"], out["fars"] = n.numpy().reshape(*out["pixel_area"].shape), f.numpy().reshape(*out["pixel_area"].shape)
    return out


def _same_nan_masks(a, b, keys):
    return [k for k in keys if not np.array_equal(np.isnan(a[k]), np.isnan(b[k]))]


# ---- the image-plane points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(54, 96), (33, 17)])
@pytest.mark.parametrize("dist", DISTORTIONS)
def test_undistorted_points_are_the_oracles_to_the_bit(dist, H, W):
    fx, fy, cx, cy = _intrinsics(H, W)
    y, x = ro.pixel_centres(H, W)
    F = np.float32
    u, v = (x - F(cx)) / F(fx), -((y - F(cy)) / F(fy))
    ux, vy = ((x - F(cx)) + F(1)) / F(fx), -(((y - F(cy)) + F(1)) / F(fy))
    for xd, yd in ((u, v), (ux, v), (u, vy)):
        got = np.stack(ro.undistort(dist, xd, yd), -1)
        want = onf.radial_and_tangential_undistort(torch.from_numpy(np.stack([xd, yd], -1)), T(dist)).numpy()
        bad = ro.diff_bits(got, want)
        print(f"{H}x{W} {dist}: {bad} of {got.size} points differ; |u| <= {np.nanmax(np.abs(got)):.3g}")
        assert bad == 0
    # and through emulate itself: "uv" of a PERSPECTIVE frame is that point
    e = ro.emulate(_c2w(0), fx, fy, cx, cy, H, W, dist)
    want = onf.radial_and_tangential_undistort(torch.from_numpy(np.stack([u, v], -1)), T(dist)).numpy().reshape(H, W, 2)
    assert ro.diff_bits(e["uv"], want) == 0


# ---- the slab tests --------------------------------------------------------------------------------------------------------------------
BOXES = {
    "hit": ro.BOX,
    "camera inside": [-3.0, -3.0, -3.0, 3.0, 3.0, 3.0],
    "missed by every ray": [5.0, 5.0, 5.0, 5.1, 5.1, 5.1],
    "zero thickness": [-0.12, 0.02, -0.08, 0.1, 0.02, 0.09],
    "inverted": [0.1, 0.12, 0.09, -0.12, -0.1, -0.08],
}


def _named_rays():
    """The issue's named rays and their kin: an origin ON a box plane with a zero direction component (0 / 0), non-finite components."""
    nan, inf = float("nan"), float("inf")
    o = [[0.1, 0, -1], [0, 0, -1], [-0.12, 0.12, -1], [0.1, 0, -1], [0, 0, -1], [0, 0, -1], [0, nan, -1], [0, 0, inf], [0.1, 0, 0], [0, 0, 0]]
    d = [[0, 0, 1], [nan, 0, 1], [0, 0, 1], [-0.0, 0, 1], [inf, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 0]]
    return ro.f32(o), ro.f32(d)


def test_slab_is_the_oracles_to_the_bit_every_nan_included():
    rays = [_named_rays()]
    for cam in CAMERAS:
        for ct in (1, 2, 3):
            e = ro.emulate(_c2w(cam), *_intrinsics(24, 40), 24, 40, DISTORTIONS[0], ct)
            rays.append((e["origins"].reshape(-1, 3), e["directions"].reshape(-1, 3)))
        eye = torch.eye(4)[:3].clone()
        eye[:, 3] = T([0.1, 0.02, 1.0])              # on the max-x plane of BOX and on the zero-thickness plane; cx = k + 0.5: exact zeros
        e = ro.emulate(eye, 30.0, 31.0, 20.5, 11.5, 24, 40)
        rays.append((e["origins"].reshape(-1, 3), e["directions"].reshape(-1, 3)))
    o, d = np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])
    for name, box in BOXES.items():
        near, far = ro.slab(o, d, box)
        for fn in (onf.intersect_aabb_ns, onf.intersect_aabb):
            wn, wf = fn(torch.from_numpy(o), torch.from_numpy(d), T(box))
            assert np.array_equal(np.isnan(near), np.isnan(wn.numpy())) and np.array_equal(np.isnan(far), np.isnan(wf.numpy())), name
            bad = ro.diff_bits(near, wn.numpy()) + ro.diff_bits(far, wf.numpy())
            print(f"{name}: {bad} of {2 * near.size} differ; {int((near < 1e10).sum())} hits, {int(np.isnan(near).sum())} NaN")
            assert bad == 0, name
    # the two rays the issue names
    near, far = ro.slab(*(a[:2] for a in _named_rays()), ro.BOX)
    assert np.isnan(near).all() and np.isnan(far).all()


def test_obb_slab_is_the_oracles_given_the_same_box_frame_rays():
    """``onf.intersect_obb`` moves the rays into the box frame with two matrix products (a BLAS call whose accumulation order is its own) and an
    fp32 inverse; the kernel uses the written ``((m0*o0 + m1*o1) + m2*o2) + m3`` and the fp32 rounding of a float64 inverse.  Given the SAME
    box-frame rays the slab test is the oracle's to the bit; the transform itself is checked for accuracy, against float64."""
    R, Tr, S = (T(ro.f32(v)) for v in ro.OBB)
    e = ro.emulate(_c2w(3), *_intrinsics(54, 96), 54, 96, DISTORTIONS[0])
    named = _named_rays()
    o = torch.from_numpy(np.concatenate([e["origins"].reshape(-1, 3), named[0]]))
    d = torch.from_numpy(np.concatenate([e["directions"].reshape(-1, 3), named[1]]))
    Hm = torch.eye(4)
    Hm[:3, :3], Hm[:3, 3] = R, Tr
    w2b = torch.inverse(Hm)
    ob = torch.matmul(w2b, torch.cat((o, torch.ones_like(o[:, :1])), -1).T).T[:, :3]
    db = torch.matmul(w2b[:3, :3], d.T).T
    for size in (S, T([0.3, 0.0, 0.2]), T([0.0, 0.0, 0.0]), T([float("nan"), 0.25, 0.2]), T([float("inf"), 0.25, 0.2])):
        wn, wf = onf.intersect_obb(o, d, R, Tr, size)
        half = ro.f32(size.numpy()) / np.float32(2)
        near, far = ro.slab(ob.numpy(), db.numpy(), np.concatenate([-half, half]))
        bad = ro.diff_bits(near, wn.numpy()) + ro.diff_bits(far, wf.numpy())
        print(f"S = {size.tolist()}: {bad} of {2 * near.size} differ; {int((near < 1e10).sum())} hits, {int(np.isnan(near).sum())} NaN")
        assert bad == 0
    # the whole of slab_obb (kernel order, the shim's world2box) against float64, where emulation, oracle and float64 agree on hit / miss
    fin = slice(0, 54 * 96)
    wn, wf = (a.numpy()[fin] for a in onf.intersect_obb(o, d, R, Tr, S))
    w = ro.world2box(R.numpy(), Tr.numpy())
    near, far = (a[fin] for a in ro.slab_obb(o.numpy(), d.numpy(), w, S.numpy()))
    tn, tf = (a[fin] for a in ro.slab_obb(o.numpy(), d.numpy(), w, S.numpy(), np.float64))
    hit = (near < 1e10) & (wn < 1e10) & (tn < 1e10)
    flips = int(((near < 1e10) != (tn < 1e10)).sum()), int(((wn < 1e10) != (tn < 1e10)).sum())
    e_emu = max(ro.max_err(near[hit], tn[hit]), ro.max_err(far[hit], tf[hit]))
    e_ora = max(ro.max_err(wn[hit], tn[hit]), ro.max_err(wf[hit], tf[hit]))
    print(f"obb vs float64 on {int(hit.sum())} common hits: emulation {e_emu:.3g}, oracle {e_ora:.3g}; hit/miss flips vs float64: {flips}")
    assert hit.sum() > 1000 and e_emu <= 2 * e_ora and flips[0] <= max(2, 2 * flips[1])


# ---- directions, norm, area ------------------------------------------------------------------------------------------------------------
def _compare(kw, label, nan_counts=None):
    e, t, r = ro.emulate(**kw), ro.truth64(**kw), oracle_rays(kw)
    assert not _same_nan_masks(e, r, e.keys() & r.keys()), label
    assert not _same_nan_masks(e, t, e.keys() & r.keys()), label
    counts = {k: int(np.isnan(r[k]).sum()) for k in OUTPUTS}
    assert counts == (nan_counts or dict.fromkeys(OUTPUTS, 0)), (label, counts)
    assert ro.diff_bits(e["origins"], r["origins"]) == 0
    dd = np.abs(e["directions"] - r["directions"])
    dmax = float(np.nanmax(dd)) if dd.size > np.isnan(dd).sum() else 0.0
    share_d = float((e["directions"].view(np.int32) != r["directions"].view(np.int32)).mean())
    share_n = float((e["directions_norm"].view(np.int32) != r["directions_norm"].view(np.int32)).mean())
    with np.errstate(all="ignore"):
        rel_a = float(np.nanmax(np.abs(e["pixel_area"] - r["pixel_area"]) / r["pixel_area"]))
    print(f"{label}: directions differ in {100 * share_d:.2f} % by <= {dmax:.3g}; norm in {100 * share_n:.2f} %; pixel_area by <= {rel_a:.3g} relative")
    for k in OUTPUTS:
        ee, eo = ro.max_err(e[k], t[k]), ro.max_err(r[k], t[k])
        print(f"    {k}: error against float64: emulation {ee:.3g}, oracle {eo:.3g}")
        assert ee <= 2 * eo, (label, k, ee, eo)
    return dmax


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("ctype", [1, 2, 3])
def test_rays_against_oracle_and_float64(ctype, cam):
    H, W = 54, 96
    for i, dist in enumerate(LENSES):
        kw = dict(c2w=_c2w(cam), H=H, W=W, dist=dist, ctype=ctype)
        kw["fx"], kw["fy"], kw["cx"], kw["cy"] = _intrinsics(H, W)
        dmax = _compare(kw, f"type {ctype} camera {cam} lens {i} {H}x{W}")
        if ctype == 1:
            assert dmax <= 1.2e-7
    # explicit coords: fractional and outside the image
    g = np.random.RandomState(7)
    coords = (g.rand(6, 50, 2) * 1.5 - 0.25) * np.float32([H, W])
    kw["coords"], kw["dist"] = coords, DISTORTIONS[0]
    dmax = _compare(kw, f"type {ctype} camera {cam} coords")
    if ctype == 1:
        assert dmax <= 1.2e-7


@pytest.mark.parametrize("i", [0, 1, 4])
def test_perspective_270x480(i):
    kw = dict(c2w=_c2w(3), H=270, W=480, dist=LENSES[i])
    kw["fx"], kw["fy"], kw["cx"], kw["cy"] = _intrinsics(270, 480)
    assert _compare(kw, f"type 1 camera 3 lens {i} 270x480") <= 1.2e-7


def test_principal_point_rays():
    """cx = k + 0.5, cy = j + 0.5: one pixel centre is the principal point.  With the identity rotation a PERSPECTIVE camera has exact-zero
    direction components there; the FISHEYE ray is 0 / 0 -- NaN direction and NaN norm in the oracle (torch.maximum keeps it), and a NaN
    pixel_area there and at the two pixels whose +1 px neighbour it is.  Nothing else is NaN for finite inputs."""
    eye = torch.eye(4)[:3].clone()
    eye[:, 3] = T([0.1, 0.0, -1.0])
    for c2w, tag in ((eye, "identity"), (_c2w(3), "camera 3")):
        kw = dict(c2w=c2w, fx=30.0, fy=31.0, cx=20.5, cy=11.5, H=24, W=40, aabb=ro.BOX)
        dmax = _compare(dict(kw, ctype=1), f"principal point, PERSPECTIVE, {tag}")
        assert dmax <= 1.2e-7
        e = ro.emulate(**kw)
        if tag == "identity":
            assert e["directions"][11, 20].tolist() == [0.0, 0.0, -1.0] and int((e["directions"] == 0).sum()) == 24 + 40
            r = oracle_rays(kw)
            assert not _same_nan_masks(e, r, ("nears", "fars")) and int(np.isnan(e["nears"]).sum()) == 24   # column 20: 0 / 0 on the max-x plane
        _compare(dict(kw, ctype=2), f"principal point, FISHEYE, {tag}", {"origins": 0, "directions": 3, "pixel_area": 3, "directions_norm": 1})
        _compare(dict(kw, ctype=3), f"principal point, EQUIRECTANGULAR, {tag}")


# ---- non-finite and degenerate inputs: the NaN pattern the GPU tests expect is the oracle's -----------------------------------------------
def test_nonfinite_inputs_have_the_oracles_nan_masks():
    cases = ro.nonfinite_cases(_c2w(3).numpy())
    refused, bad = [], []
    for name, kw in cases:
        try:
            e = ro.emulate(**kw)
        except RuntimeError:          # torch.linalg.inv refuses the pose: the Python shim refuses it the same way, before any launch
            refused.append(name)
            continue
        r = oracle_rays(kw)
        miss = _same_nan_masks(e, r, r.keys())
        if miss:
            bad.append((name, miss))
    print(f"{len(cases)} cases, {len(refused)} refused by the inverse: {refused}")
    assert not bad, bad
    assert refused == [f"obb.T[2]=inf/type{t}/plain" for t in (1, 2, 3)]
