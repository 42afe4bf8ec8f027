"""Two restatements of the camera-ray arithmetic (``sn_camera_ray`` with ``sn_undistort`` / ``sn_cam_dir``, signerf_amd/csrc/sn_stage.h, and the
clamped slab tests behind ``aabb_box`` / ``obb_box``) for the ray tests -- a helper, no tests in it.

``emulate``  numpy float32 throughout, one numpy operation per kernel operation, in the kernel's written operand order:
             ``(x - cx) / fx`` and ``((x - cx) + 1) / fx``; the 10 Newton steps with the ``|den| > 1e-3`` select; ``(a*R0 + b*R1) + c*R2``;
             ``sqrt((w0^2 + w1^2) + w2^2)`` floored at 2^-50 with NaN kept; the three divisions; the area as ``sqrt(a) * sqrt(b)`` of
             left-to-right sums; the slab as running ``np.maximum`` / ``np.minimum`` (both hand a NaN on), the clamp to [0, 1e10] and
             ``tmax <= tmin -> 1e10``.  For PERSPECTIVE cameras every operation is a correctly rounded IEEE one on both sides, so the
             kernel must equal it bit for bit.  FISHEYE / EQUIRECTANGULAR go through ``np.sin`` / ``np.cos`` on float32, which the device
             library need not match to the bit: those lenses are compared against ``truth64``.
``truth64``  the same geometry in float64 from the same fp32 inputs (and libm's float64 sin / cos): the accuracy reference.

tests/test_ray_oracle_host.py pins ``emulate`` to the CPU oracle (oracle/nerfacto.py), so "the GPU equals the emulation" means "the GPU does the
oracle's arithmetic" -- up to the one thing the two do differently, the accumulation order inside the norm (see that file).

Zero signs: ``fmaxf(t, 0)`` on the device is v_max_f32, which orders -0 below +0, while numpy's and torch's maximum return either zero.
The clamp is therefore written ``where(t <= 0, +0, t)``: a -0 plane distance (an origin ON a box plane) leaves as +0, as on the device.
"""
import math

import numpy as np

F = np.float32
PI32 = F(3.14159265358979323846)
EPS32 = F(8.8817841970012523e-16)   # 2^-50: nerfstudio's camera_utils._EPS, exact in fp32
BOUND = F(1e10)
PERSPECTIVE, FISHEYE, EQUIRECTANGULAR = 1, 2, 3


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def has_distortion(dist, ctype=PERSPECTIVE):
    """The launch rule of the Python shim and of the oracle: any parameter != 0 (so -0.0 is "none", a NaN is "some")."""
    return dist is not None and ctype != EQUIRECTANGULAR and bool(np.any(np.asarray(dist, dtype=np.float32) != 0))


def pixel_centres(H, W):
    """(y, x) of a full frame in the kernel's flat order i -> (i / W, i % W), each + 0.5."""
    iy, ix = np.divmod(np.arange(H * W, dtype=np.int64), W)
    return iy.astype(F) + F(0.5), ix.astype(F) + F(0.5)


# ---- sn_undistort --------------------------------------------------------------------------------------------------------------------
def _newton(kk, xd, yd, two, three, four, six, one, zero, eps):
    k1, k2, k3, k4, p1, p2 = kk
    x, y = xd, yd
    for _ in range(10):
        r = x * x + y * y
        d = one + r * (k1 + r * (k2 + r * (k3 + r * k4)))
        fx = ((d * x + ((two * p1) * x) * y) + p2 * (r + (two * x) * x)) - xd
        fy = ((d * y + ((two * p2) * x) * y) + p1 * (r + (two * y) * y)) - yd
        d_r = k1 + r * (two * k2 + r * (three * k3 + (r * four) * k4))
        d_x = (two * x) * d_r
        d_y = (two * y) * d_r
        fx_x = ((d + d_x * x) + (two * p1) * y) + (six * p2) * x
        fx_y = (d_y * x + (two * p1) * x) + (two * p2) * y
        fy_x = (d_x * y + (two * p2) * y) + (two * p1) * x
        fy_y = ((d + d_y * y) + (two * p2) * x) + (six * p1) * y
        den = fy_x * fx_y - fx_x * fy_y
        xn = fx * fy_y - fy * fx_y
        yn = fy * fx_x - fx * fy_x
        ok = np.abs(den) > eps
        x = x + np.where(ok, xn / den, zero)
        y = y + np.where(ok, yn / den, zero)
    return x, y


def undistort(dist, xd, yd):
    """``sn_undistort`` on float32 arrays: -> (x, y) float32."""
    kk = [F(v) for v in np.asarray(dist, dtype=np.float32).reshape(6)]
    with np.errstate(all="ignore"):
        x, y = _newton(kk, f32(xd), f32(yd), F(2), F(3), F(4), F(6), F(1), F(0), F(1e-3))
    assert x.dtype == np.float32 and y.dtype == np.float32
    return x, y


def _undistort64(dist, xd, yd):
    kk = [float(F(v)) for v in np.asarray(dist, dtype=np.float32).reshape(6)]
    with np.errstate(all="ignore"):
        return _newton(kk, xd, yd, 2.0, 3.0, 4.0, 6.0, 1.0, 0.0, float(F(1e-3)))


# ---- sn_cam_dir ----------------------------------------------------------------------------------------------------------------------
def _cam_dir(R, u, v, ctype, T):
    """T = np.float32 or np.float64 -> (directions [n,3], norm [n])."""
    pi = PI32 if T is F else math.pi
    a, b, c = u, v, np.full_like(u, -1)
    if ctype == FISHEYE:
        th = np.sqrt(u * u + v * v)
        # the clip bound is the fp32 constant on both sides (a threshold, like 1e-3).  A NaN angle has a NaN u or v, which makes every
        # output NaN whether the clip keeps the NaN (torch.clip, here) or maps it to 0 (fminf / fmaxf in the kernel)
        th = np.minimum(np.maximum(th, T(0)), T(PI32))
        st = np.sin(th)
        a = (u * st) / th
        b = (v * st) / th
        c = -np.cos(th)
    elif ctype == EQUIRECTANGULAR:
        theta, phi = T(-pi) * u, T(pi) * (T(0.5) - v)
        sp = np.sin(phi)
        a = (-np.sin(theta)) * sp
        b = np.cos(phi)
        c = (-np.cos(theta)) * sp
    elif ctype != PERSPECTIVE:
        raise ValueError(ctype)
    w = [(a * R[i, 0] + b * R[i, 1]) + c * R[i, 2] for i in range(3)]
    n = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    n = np.maximum(n, T(EPS32))                        # np.maximum keeps a NaN norm, as torch.maximum does
    return np.stack([w[0] / n, w[1] / n, w[2] / n], -1), n


# ---- the clamped slab tests ----------------------------------------------------------------------------------------------------------
def _clamp(t, T):
    t = np.where(t <= T(0), T(0), t)                   # fmaxf(t, 0) with -0 < +0; a NaN stays
    return np.where(t >= T(BOUND), T(BOUND), t)


def _slab_finish(lo, hi, T):
    tmin, tmax = np.full_like(lo[0], -np.inf), np.full_like(lo[0], np.inf)
    for a, b in zip(lo, hi):
        tmin = np.maximum(tmin, np.minimum(a, b))
        tmax = np.minimum(tmax, np.maximum(a, b))
    tmin, tmax = _clamp(tmin, T), _clamp(tmax, T)
    miss = tmax <= tmin
    return np.where(miss, T(BOUND), tmin), np.where(miss, T(BOUND), tmax)


def slab(origins, directions, aabb, T=F):
    """nerfstudio's intersect_aabb as ``sn_camera_ray`` does it with ``want_box``: origins / directions [n,3], aabb [6] -> nears, fars [n]."""
    o, d, box = np.asarray(origins, dtype=T).reshape(-1, 3), np.asarray(directions, dtype=T).reshape(-1, 3), np.asarray(aabb, dtype=T).reshape(6)
    with np.errstate(all="ignore"):
        lo = [(box[c] - o[:, c]) / d[:, c] for c in range(3)]
        hi = [(box[3 + c] - o[:, c]) / d[:, c] for c in range(3)]
        return _slab_finish(lo, hi, T)


def world2box(R, T):
    """The 3x4 fp32 world-to-box matrix the Python shim hands to ``sn_intersect_obb``: the float64 inverse of [R | T], rounded."""
    import torch

    pose = torch.eye(4, dtype=torch.float64)
    pose[:3, :3] = torch.from_numpy(f32(R)).to(torch.float64)
    pose[:3, 3] = torch.from_numpy(f32(T)).to(torch.float64).reshape(3)
    return torch.linalg.inv(pose)[:3].to(torch.float32).numpy()


def slab_obb(origins, directions, w2b, size, T=F):
    """``sn_intersect_obb_kernel``: rays into the box frame by the 3x4 ``w2b``, then the slab test against [-S/2, S/2]."""
    o, d = np.asarray(origins, dtype=T).reshape(-1, 3), np.asarray(directions, dtype=T).reshape(-1, 3)
    m = np.asarray(f32(w2b).reshape(3, 4), dtype=T)
    with np.errstate(all="ignore"):
        half = np.asarray(f32(size).reshape(3) / F(2), dtype=T)
        lo, hi = [], []
        for c in range(3):
            ob = ((m[c, 0] * o[:, 0] + m[c, 1] * o[:, 1]) + m[c, 2] * o[:, 2]) + m[c, 3]
            db = (m[c, 0] * d[:, 0] + m[c, 1] * d[:, 1]) + m[c, 2] * d[:, 2]
            lo.append((-half[c] - ob) / db)
            hi.append((half[c] - ob) / db)
        return _slab_finish(lo, hi, T)


# ---- sn_camera_ray -------------------------------------------------------------------------------------------------------------------
def _rays(T, c2w, fx, fy, cx, cy, H, W, dist, ctype, coords, aabb, obb):
    c2w = np.asarray(f32(c2w)[:3, :4], dtype=T)
    fx, fy, cx, cy = (T(F(v)) for v in (fx, fy, cx, cy))
    if coords is None:
        y, x = pixel_centres(H, W)
        shape = (H, W)
    else:
        coords = f32(coords)
        shape = coords.shape[:-1]
        y, x = coords.reshape(-1, 2)[:, 0], coords.reshape(-1, 2)[:, 1]
    y, x = np.asarray(y, dtype=T), np.asarray(x, dtype=T)
    with np.errstate(all="ignore"):
        u, v = (x - cx) / fx, -((y - cy) / fy)
        ux, vx = ((x - cx) + T(1)) / fx, v
        uy, vy = u, -(((y - cy) + T(1)) / fy)
        if has_distortion(dist, ctype):
            und = undistort if T is F else _undistort64
            u0, v0 = u, v
            u, v = und(dist, u0, v0)
            ux, vx = und(dist, ux, v0)
            uy, vy = und(dist, u0, vy)
        d, n = _cam_dir(c2w, u, v, ctype, T)
        dx, _ = _cam_dir(c2w, ux, vx, ctype, T)
        dy, _ = _cam_dir(c2w, uy, vy, ctype, T)
        e, f = d - dx, d - dy
        a = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        b = (f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]
        area = np.sqrt(a) * np.sqrt(b)
    o = np.broadcast_to(c2w[:, 3], d.shape).copy()
    out = {"origins": o.reshape(*shape, 3), "directions": d.reshape(*shape, 3), "pixel_area": area.reshape(*shape, 1),
           "directions_norm": n.reshape(*shape, 1), "uv": np.stack([u, v], -1).reshape(*shape, 2)}
    if aabb is not None:
        nr, fr = slab(o, d, f32(aabb).reshape(6), T)
    elif obb is not None:
        R, Tr, S = obb
        nr, fr = slab_obb(o, d, world2box(R, Tr), S, T)
    if aabb is not None or obb is not None:
        out["nears"], out["fars"] = nr.reshape(*shape, 1), fr.reshape(*shape, 1)
    for k, val in out.items():
        assert val.dtype == T, (k, val.dtype)
    return out


def emulate(c2w, fx, fy, cx, cy, H=None, W=None, dist=None, ctype=PERSPECTIVE, coords=None, aabb=None, obb=None):
    """``sn_camera_ray<ctype, dist != 0>`` for a full H x W frame or for explicit ``coords`` [..., 2] = (y, x), in numpy float32.
    ``aabb`` [6] | [2,3] adds nears / fars of the slab test inside the ray kernel, ``obb`` = (R, T, S) those of ``sn_intersect_obb`` (``aabb``
    wins, as in ``Cameras.generate_rays``).  -> dict of float32 arrays shaped like the bundle, plus "uv" (the un-distorted image-plane point)."""
    return _rays(F, c2w, fx, fy, cx, cy, H, W, dist, ctype, coords, aabb, obb)


def truth64(c2w, fx, fy, cx, cy, H=None, W=None, dist=None, ctype=PERSPECTIVE, coords=None, aabb=None, obb=None):
    """The same geometry in float64 from the same fp32 inputs."""
    return _rays(np.float64, c2w, fx, fy, cx, cy, H, W, dist, ctype, coords, aabb, obb)


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
def diff_bits(a, b):
    """Number of elements that differ: another NaN pattern, or other bits where neither is NaN."""
    a, b = f32(a), f32(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(np.int32) != b.view(np.int32)))).sum())


def max_err(a, truth):
    """max |a - truth| over the elements whose truth is not NaN (0 when there is none); inf - inf counts as 0, a stray NaN as inf."""
    a, t = np.asarray(a, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    keep = ~np.isnan(t)
    if not keep.any():
        return 0.0
    with np.errstate(all="ignore"):
        e = np.where(a[keep] == t[keep], 0.0, np.abs(a[keep] - t[keep]))
    return float(np.where(np.isnan(e), np.inf, e).max())


# ---- the non-finite and degenerate inputs of tests/test_gpu_ray_edges.py part D, shared with tests/test_ray_oracle_host.py -----------------
NAN, INF = float("nan"), float("inf")
LENS = [0.05, -0.02, 0.0, 0.0, 0.001, -0.002]          # DISTORTIONS[0] of tests/test_gpu_cameras.py
BOX = [-0.12, -0.1, -0.08, 0.1, 0.12, 0.09]
OBB_R = [[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]   # a rotation with exact fp32-friendly entries (3-4-5 triangles)
OBB = (OBB_R, [0.02, -0.01, 0.03], [0.3, 0.25, 0.2])


def nonfinite_cases(c2w):
    """-> list of (name, kwargs of emulate / of the tests' ``run``): one non-finite or degenerate input each, on a 5 x 7 frame (35 rays, or the
    explicit coords), for every lens the input applies to.  ``c2w`` [3,4]: a general finite pose."""
    c2w = f32(c2w)[:3, :4]
    base = dict(c2w=c2w, fx=6.5, fy=6.25, cx=3.5, cy=2.25, H=5, W=7, dist=None, coords=None, aabb=BOX, obb=None)
    coords = [[NAN, 1.5], [2.5, NAN], [INF, 1.0], [1.0, -INF], [1e30, 2.0], [3.0, 1e30], [-1e30, -1e30], [NAN, NAN], [2.5, 3.5]]
    out = []

    def add(name, lenses=(PERSPECTIVE, FISHEYE, EQUIRECTANGULAR), distorted=(False, True), **kw):
        for ct in lenses:
            for dd in distorted:
                if dd and ct == EQUIRECTANGULAR:
                    continue
                case = dict(base, ctype=ct, **kw)
                if dd and case["dist"] is None:
                    case["dist"] = LENS
                if not dd and case["dist"] is not None:
                    continue
                out.append((f"{name}/type{ct}/{'dist' if dd else 'plain'}", case))

    for tag, v in (("nan", NAN), ("+inf", INF), ("-inf", -INF)):
        m = c2w.copy(); m[0, 1] = v
        add(f"rotation[0,1]={tag}", c2w=m)
        m = c2w.copy(); m[2, 2] = v
        add(f"rotation[2,2]={tag}", c2w=m, distorted=(False,))
        m = c2w.copy(); m[1, 3] = v
        add(f"translation[1]={tag}", c2w=m)
        m = c2w.copy(); m[1, 3] = v
        add(f"translation[1]={tag}/obb", c2w=m, aabb=None, obb=OBB, distorted=(False,))
    add("fx=0", fx=0.0)
    add("fx=inf", fx=INF)
    add("fy=-0", fy=-0.0, distorted=(False,))
    add("cx=nan", cx=NAN)
    add("cy=inf", cy=INF, distorted=(False,))
    add("coords", coords=coords)
    add("coords/obb", coords=coords, aabb=None, obb=OBB, distorted=(False,))
    for tag, v in (("nan", NAN), ("inf", INF), ("1e30", 1e30), ("-1e30", -1e30)):
        for slot in (0, 3, 4):
            d = [0.0] * 6; d[slot] = v
            add(f"dist[{slot}]={tag}", lenses=(PERSPECTIVE, FISHEYE), distorted=(True,), dist=d)
        d = list(LENS); d[1] = v
        add(f"lens+dist[1]={tag}", lenses=(PERSPECTIVE, FISHEYE), distorted=(True,), dist=d)
    for tag, v in (("nan", NAN), ("+inf", INF), ("-inf", -INF)):
        for slot in (0, 4):
            b = list(BOX); b[slot] = v
            add(f"aabb[{slot}]={tag}", aabb=b, distorted=(False,))
    add("aabb=all-inf", aabb=[-INF] * 3 + [INF] * 3, distorted=(False,))
    add("aabb=all-nan", aabb=[NAN] * 6, lenses=(PERSPECTIVE,), distorted=(False,))
    for tag, v in (("nan", NAN), ("inf", INF)):
        t = list(OBB[1]); t[2] = v
        add(f"obb.T[2]={tag}", aabb=None, obb=(OBB_R, t, OBB[2]), distorted=(False,))
        sz = list(OBB[2]); sz[0] = v
        add(f"obb.S[0]={tag}", aabb=None, obb=(OBB_R, OBB[1], sz), distorted=(False,))
        r = [list(row) for row in OBB_R]; r[1][1] = v
        add(f"obb.R[1,1]={tag}", aabb=None, obb=(r, OBB[1], OBB[2]), lenses=(PERSPECTIVE,), distorted=(False,))
    add("obb.S=0", aabb=None, obb=(OBB_R, OBB[1], [0.0, 0.0, 0.0]), distorted=(False,))
    add("obb.S[1]=0", aabb=None, obb=(OBB_R, OBB[1], [0.3, 0.0, 0.2]), distorted=(False,))
    return out


def gate_failures(got, oracle, truth):
    """The accuracy gate of the lenses that go through sin / cos: per element |got - truth| <= 2 * max|oracle - truth| + one ulp of the
    element, the yardstick being the oracle's own maximum error on the same case.  An element whose truth is NaN is left out (the NaN
    masks are compared separately).  -> (number of failing elements, max |got - truth|, the yardstick max|oracle - truth|)."""
    g, t = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    keep = ~np.isnan(t)
    yard = max_err(oracle, truth)
    with np.errstate(all="ignore"):
        err = np.where(g == t, 0.0, np.abs(g - t))
        err = np.where(np.isnan(err), np.inf, err)
        ulp = np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
        ulp = np.where(np.isfinite(ulp), ulp, 0.0)
        bad = keep & ~(err <= 2.0 * yard + ulp)
    return int(bad.sum()), (float(err[keep].max()) if keep.any() else 0.0), yard
