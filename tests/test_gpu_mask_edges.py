"""The mask step at the sizes, element shapes and inputs the other mask tests never reach (``sn_aabb_mask_condition``,
``sn_shape_mask_condition``, ``sn_aabb_mask_condition_combined``), every comparison bit-exact: the mask by ``torch.equal``, the condition
by NaN pattern + bits (boolean work and strict IEEE arithmetic: there is no tolerance to choose).  Each test prints its figures first.

A. Production sizes.  The visible kernels are grid-stride kernels capped at 512 workgroups x 256 threads = 131 072 pixels per sweep, so a
   thread loops a second time only above that size -- all other oracle comparisons of the suite are at or below 19 200 pixels.  Here: 800x800
   and 1080x1920 frames, exactly 131 072 and 131 073 pixels, one-row / one-column images and widths either side of a 64-pixel prefix chunk.
   The scenes put the statistics' extremes (the depth minimum / maximum the condition is normalised by) at flat indices only a LATER sweep
   sees, so a kernel that loses the carried count / min / max gets dmin / dmax wrong.  Plus: determinism, and a call sequence on memory the
   allocator hands back (visible, nothing visible, the first again).
B. Every structuring-element shape by its impulse response (tests/test_mask_oracle_host.py pins the construction against the oracle's
   dilate): all (w, h) of [1..32]^2 and the sizes around 50 / 64 / 128 / 256, unclipped and clipped on every side; the refusals.
C. Non-finite rays and depths in the aabb and combined modes and in ``sn_intersect_with_aabb``.  The reference's slab test is
   torch.minimum / maximum / max / min, which hand a NaN on; before this file the kernels used fminf / fmaxf alone, which drop it.  What
   disagreed then (measured on an MI355X with the kernels as they were): a NaN direction component and a NaN origin component of a ray that
   hits the box on its other two axes -- the kernel called the patch pixel visible, the oracle does not; 6 of the 48 mask cases failed,
   both kinds undilated with and without inverse_mask and dilated under inverse_mask (dilated and uninverted, the patch around the pixel
   covers it) -- and, in sn_intersect_with_aabb, those two plus d == -1e-6f with the origin on a box plane (0 * inf: finite / +inf where
   the oracle has NaN; the mask agreed there, a +inf near being invisible too).  +-inf direction components, d == -1e-6f off the plane
   and all non-finite / zero / negative depths agreed.  The kernels now share ``sn_aabb_slab``, which hands the NaN on.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import mesh_color_oracle as mco
import mesh_oracle as mo
from oracle import nerfacto as onf
from oracle import signerf_utils as su
from signerf_amd import _lib, intersect_with_aabb, scene
from signerf_amd.datasetgenerator import aabb_mask_and_condition, aabb_mask_and_condition_combined, shape_mask_and_condition
from test_mask_oracle_host import border_points, impulse_response

pytestmark = pytest.mark.gpu

SWEEP = 512 * 256   # SN_MASK_VIS_BLOCKS workgroups of 256 threads: a pixel whose flat index is >= SWEEP is seen by a later loop iteration only
AABB = torch.tensor([[-0.1, -0.1, -0.1], [0.1, 0.1, 0.1]])
NOWHERE = torch.tensor([[5.0, 5.0, 5.0], [5.1, 5.1, 5.1]])   # a box no ray meets
MODES = ["aabb", "shape", "combined"]


@pytest.fixture(scope="module", autouse=True)
def shared_oracle_dilations():
    """The oracle's dilate is most of this file's time (8 s per 1080p frame with the 50x50 element) and the modes, the with/without-condition
    calls and the manual-depth case ask it for the same dilation again: answered once per distinct (image, element), by content."""
    real, cache = su.dilate, {}

    def cached(src, elem):
        key = (src.shape, elem.shape, src.dtype.str, hashlib.blake2b(np.ascontiguousarray(src).tobytes(), digest_size=16).digest(),
               hashlib.blake2b(np.ascontiguousarray(elem).tobytes(), digest_size=16).digest())
        if key not in cache:
            cache[key] = real(src, elem)
        return cache[key].copy()

    su.dilate = cached
    yield
    su.dilate = real


def _diff_bits(a, b):
    """Number of elements that differ: another NaN pattern, or other bits where neither is NaN (0 <=> the ``_same_bits`` idiom holds)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(torch.int32) != b.view(torch.int32)))).sum())


def _late(n):
    """(flat indices that may hold the maximum, ... the minimum): beyond the first sweep where the image has such pixels.  With exactly
    SWEEP + 1 pixels ONE pixel is left for the second sweep, so only the maximum can sit there."""
    flat = torch.arange(n)
    if n <= SWEEP:
        return flat >= 0, flat >= 0
    late = flat >= SWEEP
    return late, (late if n > SWEEP + 1 else flat >= 0)


# ---- scenes: tests/test_gpu_mask.py::_scene, tests/test_gpu_shape_mask.py::_depths and tests/test_gpu_mesh_color.py::_scene, extended to
# one-row / one-column images and with the statistics' extremes placed ---------------------------------------------------------------------
def _rays(H, W):
    f = 1.4 * max(H, W)
    r = onf.generate_rays(scene.benchmark_cameras(8)[1, :3], f, f, W / 2, H / 2, H, W)
    return r["origins"].clone(), r["directions"].clone()


def _aabb_scene(H, W, place=True):
    """-> origins, directions, depth, (flat index of the visible depth minimum, ... maximum) | None."""
    o, d = _rays(H, W)
    n = H * W
    if n == SWEEP + 1:   # the single pixel of the second sweep looks at the box: it gets the centre ray
        o[-1, -1], d[-1, -1] = o[H // 2, W // 2].clone(), d[H // 2, W // 2].clone()
    g = torch.Generator().manual_seed(n + 1)
    depth = 2.0 + torch.rand(H, W, 1, generator=g)   # far background with one patch (plus isolated pixels) whose depth falls inside the box
    y0, x0 = (3 * H) // 8, (3 * W) // 8
    y1, x1 = max((5 * H) // 8, y0 + 1), max((5 * W) // 8, x0 + 1)
    depth[y0:y1, x0:x1] = 0.45 + 0.1 * torch.rand(y1 - y0, x1 - x0, 1, generator=g)
    if W > 2:
        depth[H // 2, 1] = 0.5
    if H > 2:
        depth[1, W // 2] = 0.5
    if not place:
        return o, d, depth, None
    # the extremes: just behind the smallest near and just before the largest far among the rays a later sweep owns, so that they are
    # visible and lie outside the patch's [0.45, 0.55]
    nears, fars = su.intersect_with_aabb(o, d, AABB)
    nears, fars = nears.reshape(-1), fars.reshape(-1)
    hit = (nears < fars) & (nears > 0)
    late_max, late_min = _late(n)
    i_min = int(torch.where(hit & late_min, nears, torch.full_like(nears, float("inf"))).argmin())
    fm = torch.where(hit & late_max, fars, torch.full_like(fars, -float("inf")))
    fm[i_min] = -float("inf")
    i_max = int(fm.argmax())
    flat = depth.view(-1)
    flat[i_min], flat[i_max] = nears[i_min] * 1.01, fars[i_max] * 0.99
    assert hit[i_min] and hit[i_max] and i_min != i_max
    assert nears[i_min] < flat[i_min] < min(float(fars[i_min]), 0.45) and max(float(nears[i_max]), 0.55) < flat[i_max] < fars[i_max]
    return o, d, depth, (i_min, i_max)


def _ellipse(H, W, cy, cx, ry, rx):
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1.0


def _shape_scene(H, W, mesh=True):
    """-> mesh depth, NeRF depth, (flat index of the visible mesh-depth minimum, ... of the mesh-depth maximum) | None."""
    n = H * W
    g = torch.Generator().manual_seed(n)
    nerf = 2.0 + torch.rand(H, W, 1, generator=g)
    md = torch.zeros(H, W, 1)
    if not mesh:
        return md, nerf, None
    disc = _ellipse(H, W, (H - 1) / 2, (W - 1) / 2, max(H / 5, 1.0), max(W / 5, 1.0))
    md[..., 0][disc] = 0.5 + 0.2 * torch.rand(int(disc.sum()), generator=g)
    nerf[: H // 2, : W // 2] = 0.55   # the NeRF occludes part of the mesh
    if H > 2 and W > 2:
        md[1, 1] = 0.6                # an isolated mesh pixel
    vis = ((md > 0) & (md < nerf)).view(-1)
    i_min = int(torch.nonzero(vis).max())   # the last visible mesh pixel; the maximum (taken over EVERY mesh pixel) goes on the last pixel
    i_max = n - 1
    assert i_min != i_max
    md.view(-1)[i_min], md.view(-1)[i_max] = 0.45, 0.75
    return md, nerf, (i_min, i_max)


def _combined_extras(H, W):
    """The mesh of the combined mode: a disc that overlaps the box patch and the background, in front of the NeRF in places, behind in others."""
    g = torch.Generator().manual_seed(H * W + 7)
    disc = _ellipse(H, W, 0.45 * (H - 1), 0.55 * (W - 1), max(H / 3.5, 1.0), max(W / 3.5, 1.0))
    md = torch.zeros(H, W, 1)
    md[..., 0][disc] = 0.3 + 0.4 * torch.rand(int(disc.sum()), generator=g)
    color = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    return md, color


def _inputs(mode, H, W, visible=True):
    """-> (tensors the entry point takes, in the order of its wrapper AND of its oracle; box | None; placed extremes | None; the combined
    mode's [mesh depth, mesh colour]).  visible=False: the same scene with nothing visible (no mesh / a box no ray meets)."""
    if mode == "shape":
        md, nerf, ext = _shape_scene(H, W, mesh=visible)
        return [md, nerf], None, ext, []
    o, d, depth, ext = _aabb_scene(H, W)
    extras = list(_combined_extras(H, W)) if mode == "combined" else []
    return [depth, o, d], (AABB if visible else NOWHERE), (ext if visible else None), extras


def _gpu_call(mode, gpu, t, box, extras, dil, inverse=False, manual=None, with_condition=True):
    t = [x.to(gpu) for x in t]
    if mode == "shape":
        return shape_mask_and_condition(t[0], t[1], dil, inverse, manual, 0.1, with_condition=with_condition)
    if mode == "aabb":
        return aabb_mask_and_condition(t[0], t[1], t[2], box, dil, inverse, manual, 0.1, with_condition=with_condition)
    return aabb_mask_and_condition_combined(t[0], t[1], t[2], box, extras[0].to(gpu), extras[1].to(gpu), dil, inverse, manual, 0.1,
                                            with_condition=with_condition)


def _oracle(mode, t, box, extras, dil, inverse=False, manual=None):
    if mode == "shape":
        return mo.shape_mask_and_condition(t[0], t[1], dil, inverse, manual, 0.1)
    if mode == "aabb":
        return su.aabb_mask_and_condition(t[0], t[1], t[2], box, dil, inverse, manual, 0.1)
    return mco.combined_mask_and_condition(t[0], t[1], t[2], box, extras[0], extras[1], dil, inverse, manual, 0.1)


def _check_against_oracle(gpu, mode, H, W, dil, inverse=False, manual=None):
    n = H * W
    t, box, ext, extras = _inputs(mode, H, W)
    mask, cond = _gpu_call(mode, gpu, t, box, extras, dil, inverse, manual)
    mask_b, cond_b = _gpu_call(mode, gpu, t, box, extras, dil, inverse, manual)                      # determinism
    mask_c, none_c = _gpu_call(mode, gpu, t, box, extras, dil, inverse, manual, with_condition=False)
    rmask, rcond = _oracle(mode, t, box, extras, dil, inverse, manual)
    rvis, _ = _oracle(mode, t, box, extras, None, False, manual)      # the undilated, uninverted visible mask
    rvis_cfg, _ = _oracle(mode, t, box, extras, None, inverse, manual)
    frac = float(rvis.float().mean())
    mask_diff, cond_diff = int((mask.cpu() != rmask).sum()), _diff_bits(cond, rcond)
    print(f"\n[A] {mode:8s} {H}x{W} = {n} pixels, element {dil}, inverse {inverse}, manual {manual}: visible fraction {frac:.4f} "
          f"({int(rvis.sum())} pixels), mask {int(rvis_cfg.sum())} -> {int(rmask.sum())} set after dilation; extremes at flat {ext} "
          f"(first sweep ends at {SWEEP}); mask mismatches {mask_diff}, condition words that differ {cond_diff}, "
          f"repeat-call differences {int((mask != mask_b).sum())} / {_diff_bits(cond, cond_b)}")
    assert mask.dtype == torch.bool and mask.shape == (H, W, 1) and cond.shape == (H, W, 1) and cond.dtype == torch.float32
    # non-vacuous: some pixels are visible, most are not, and the dilation really grows the mask
    assert 0.005 < frac < 0.5
    assert int(rmask.sum()) > int(rvis_cfg.sum())
    # the statistics' extremes are where the scene put them: in a later sweep wherever the image has one
    if ext is not None and not inverse and manual is None:
        i_min, i_max = ext
        v = rvis.view(-1)
        if mode == "shape":
            md = t[0].view(-1)
            sel = torch.where(v & (md > 0), md, torch.full_like(md, float("inf")))
            assert int(sel.argmin()) == i_min and int((sel == sel[i_min]).sum()) == 1
            assert int(md.argmax()) == i_max and int((md == md[i_max]).sum()) == 1
        else:
            z = t[0].view(-1)
            assert v[i_min] and v[i_max]
            assert int(torch.where(v, z, torch.full_like(z, float("inf"))).argmin()) == i_min and int((z[v] == z[i_min]).sum()) == 1
            assert int(torch.where(v, z, torch.full_like(z, -float("inf"))).argmax()) == i_max and int((z[v] == z[i_max]).sum()) == 1
        if n > SWEEP:
            assert i_max >= SWEEP
        if n > SWEEP + 1:
            assert i_min >= SWEEP
    if mode == "combined":
        cv = (extras[0] < t[0]) & (extras[0] > 0)
        assert int(cv.sum()) > 0 and int((~cv & (extras[0] > 0)).sum()) > 0   # the mesh is in front in places and behind in others
    assert mask_diff == 0      # BIT-EXACT mask: visibility of every pixel, dilation footprint, border handling
    assert cond_diff == 0      # strict IEEE: a wrong dmin / dmax changes every word
    assert torch.equal(mask, mask_b) and _diff_bits(cond, cond_b) == 0
    assert torch.equal(mask_c, mask) and none_c is None


SIZES_A = [
    (800, 800, (50, 50)),      # production frame
    (1080, 1920, (50, 50)),    # production frame
    (512, 256, (50, 50)),      # exactly one sweep
    (3, 43691, (50, 50)),      # one pixel more than a sweep; 683 prefix chunks per row
    (1, 300, (9, 5)),          # degenerate height
    (300, 1, (9, 5)),          # degenerate width
    (70, 63, (9, 5)),          # one pixel short of a 64-pixel prefix chunk
    (70, 64, (9, 5)),          # exactly one chunk
    (70, 65, (9, 5)),          # one pixel into the second chunk
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W,dil", SIZES_A)
def test_production_sizes_match_oracle(gpu, H, W, dil, mode):
    _check_against_oracle(gpu, mode, H, W, dil)


@pytest.mark.parametrize("mode", MODES)
def test_production_frame_inverse_mask_matches_oracle(gpu, mode):
    _check_against_oracle(gpu, mode, 800, 800, (50, 50), inverse=True)


def test_production_frame_manual_depth_matches_oracle(gpu):
    _check_against_oracle(gpu, "aabb", 800, 800, (50, 50), manual=(0.1, 0.9))


@pytest.mark.parametrize("mode", MODES)
def test_call_sequence_on_recycled_memory(gpu, mode):
    """Visible, nothing visible, the first again, at 800x800: the workspace of each call is memory the allocator just took back from the
    call before, so the three statistics words hold that call's results until they are reset."""
    H = W = 800
    t, box, _, extras = _inputs(mode, H, W)
    t0, box0, _, extras0 = _inputs(mode, H, W, visible=False)
    first = _gpu_call(mode, gpu, t, box, extras, (50, 50))
    second = _gpu_call(mode, gpu, t0, box0, extras0, (50, 50))
    third = _gpu_call(mode, gpu, t, box, extras, (50, 50))
    print(f"\n[A] {mode:8s} recycled memory {H}x{W}: first mask {int(first[0].sum())} set; second mask {int(second[0].sum())} set, "
          f"condition |max| {float(second[1].abs().max())}; third vs first: mask differences {int((third[0] != first[0]).sum())}, "
          f"condition words that differ {_diff_bits(third[1], first[1])}")
    assert int(first[0].sum()) > 0.005 * H * W
    assert not bool(second[0].any()) and int((second[1].view(torch.int32) != 0).sum()) == 0     # all zeros, +0.0 at that
    assert torch.equal(third[0], first[0]) and _diff_bits(third[1], first[1]) == 0


# ---- B. every structuring-element shape, by impulse response ----------------------------------------------------------------------------
LARGE = [49, 50, 51, 63, 64, 65, 127, 128, 129, 255, 256]
ELEMENTS_SMALL = [(w, h) for w in range(1, 33) for h in range(1, 33)]
ELEMENTS_LARGE = sorted({(w, h) for w in LARGE for h in LARGE} | {(w, h) for w in LARGE for h in (1, 2, 3)} | {(w, h) for w in (1, 2, 3) for h in LARGE})


def _impulse_mismatches(gpu, H, W, points, w, h):
    """Device scalar: pixels where the shape-mode mask of the impulses `points` differs from the clipped union of reflected (w, h) elements.
    The mesh depth is the impulse image, the NeRF depth a constant behind it, so the visible mask IS the impulse image."""
    md = torch.zeros((H, W, 1), dtype=torch.float32, device=gpu)
    ys, xs = zip(*points)
    md[list(ys), list(xs)] = 0.5
    nerf = torch.full((H, W, 1), 2.0, dtype=torch.float32, device=gpu)
    mask, _ = shape_mask_and_condition(md, nerf, (w, h), with_condition=False)
    want = torch.from_numpy(impulse_response(H, W, points, su.ellipse_element(w, h))).to(gpu)
    return (mask[..., 0] != (want != 0)).sum()


@pytest.mark.parametrize("name,elements", [("every (w, h) of [1..32]^2", ELEMENTS_SMALL), ("sizes around 50 / 64 / 128 / 256", ELEMENTS_LARGE)])
def test_every_element_shape_by_impulse_response(gpu, name, elements):
    assert len(elements) == (1024 if elements is ELEMENTS_SMALL else 11 * 11 + 2 * 33)
    counts = torch.stack([_impulse_mismatches(gpu, 2 * h + 3, 2 * w + 3, [(h + 1, w + 1)], w, h) for w, h in elements]).cpu()
    bad = [(elements[i], int(counts[i])) for i in torch.nonzero(counts).view(-1).tolist()]
    even = sum(1 for w, h in elements if w % 2 == 0 or h % 2 == 0)
    print(f"\n[B] {name}: {len(elements)} elements compared ({even} with an even side, which show the reflection), "
          f"{len(elements) - len(bad)} equal; mismatching (element, pixels): {bad[:20]}")
    assert not bad


CLIPPED = [(256, 256), (255, 1), (1, 255), (2, 2), (255, 255), (256, 1), (1, 256), (50, 50), (9, 5), (64, 63), (3, 128), (127, 2), (51, 50), (2, 1)]


def test_element_clipped_on_every_side(gpu):
    """Images smaller than the element, impulses at the four corners and the four edge midpoints: all in one image (the union of the clipped
    reflections -- which covers nearly every such image completely, so an always-set mask would pass), and each impulse alone in the same
    image, which leaves pixels unset and is not symmetric.  Every clamp of the row runs to [0, width) and every skipped row outside
    [0, height) is exercised."""
    assert set(CLIPPED) <= set(ELEMENTS_SMALL) | set(ELEMENTS_LARGE)
    cases, partial = [], 0
    for w, h in CLIPPED:
        elem = su.ellipse_element(w, h)
        for H, W in sorted({(max(1, h // 2), max(1, w // 2)), (max(1, h - 1), max(1, w // 3))}):
            assert (H < h or h == 1) and (W < w or w == 1)
            pts = border_points(H, W)
            cases.append((w, h, H, W, pts))
            for p in pts:
                cases.append((w, h, H, W, [p]))
                partial += int(0 < int(impulse_response(H, W, [p], elem).sum()) < H * W)
    counts = torch.stack([_impulse_mismatches(gpu, H, W, pts, w, h) for w, h, H, W, pts in cases]).cpu()
    bad = [(cases[i], int(counts[i])) for i in torch.nonzero(counts).view(-1).tolist()]
    print(f"\n[B] clipped: {len(cases)} (element w, h, image H, W, impulses) cases over {len(CLIPPED)} elements, {partial} of them with set and "
          f"unset pixels expected, {len(cases) - len(bad)} equal; mismatching: {bad[:20]}")
    assert partial >= len(cases) // 2
    assert not bad


def test_element_sizes_and_workspace_refusals_leave_the_outputs_alone(gpu):
    """257 in either dimension, (0, 5), (5, 0): SN_ERR_INVALID; a workspace one byte short: SN_ERR_WORKSPACE; all three entry points, and
    neither output is written.  The same buffers then serve a call that is accepted."""
    lib = _lib.load()
    H, W = 24, 40
    o, d, depth, _ = _aabb_scene(H, W, place=False)
    md, color = _combined_extras(H, W)
    o, d, depth, md, color = (x.to(gpu).contiguous() for x in (o, d, depth, md, color))
    box = (C.c_float * 6)(*AABB.reshape(-1).tolist())
    need = lib.sn_mask_workspace_bytes(H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    mask = torch.full((H, W, 1), 0x5A, dtype=torch.uint8, device=gpu)
    cond = torch.full((H, W, 1), -5.0, dtype=torch.float32, device=gpu)

    def call(which, dw, dh, ws_bytes):
        opts = _lib.SnMaskOpts()
        opts.dilate_w, opts.dilate_h, opts.additional_depth_radius = dw, dh, 0.1
        tail = (_lib.ptr(mask), _lib.ptr(cond), ws.data_ptr(), ws_bytes, _lib.current_stream())
        if which == "aabb":
            return lib.sn_aabb_mask_condition(_lib.ptr(o), _lib.ptr(d), _lib.ptr(depth), H, W, box, C.byref(opts), *tail)
        if which == "shape":
            return lib.sn_shape_mask_condition(_lib.ptr(md), _lib.ptr(depth), H, W, C.byref(opts), *tail)
        return lib.sn_aabb_mask_condition_combined(_lib.ptr(o), _lib.ptr(d), _lib.ptr(depth), H, W, box, C.byref(opts), _lib.ptr(md),
                                                   _lib.ptr(color), *tail)

    seen = []
    for which in MODES:
        for dw, dh, ws_bytes, want in ((257, 5, need, _lib.SN_ERR_INVALID), (5, 257, need, _lib.SN_ERR_INVALID), (257, 257, need, _lib.SN_ERR_INVALID),
                                       (0, 5, need, _lib.SN_ERR_INVALID), (5, 0, need, _lib.SN_ERR_INVALID), (5, 5, need - 1, _lib.SN_ERR_WORKSPACE),
                                       (0, 0, need - 1, _lib.SN_ERR_WORKSPACE)):
            st = call(which, dw, dh, ws_bytes)
            torch.cuda.synchronize()
            untouched = bool((mask == 0x5A).all()) and bool((cond == -5.0).all())
            seen.append((which, dw, dh, ws_bytes - need, st, untouched))
            assert st == want and untouched, seen[-1]
    print(f"\n[B] refusals (entry point, w, h, workspace bytes - needed, status, outputs untouched): {seen}")
    for which in MODES:     # ... and the largest element is accepted, with exactly the workspace asked for
        mask.fill_(0x5A)
        assert call(which, 256, 256, need) == _lib.SN_OK
        torch.cuda.synchronize()
        assert bool((mask <= 1).all()) and bool(mask.any()) and not bool((cond == -5.0).any())


# ---- C. non-finite inputs, aabb and combined modes ------------------------------------------------------------------------------------
HC, WC = 64, 80
P_IN, P_BG = (HC // 2 + 2, WC // 2 + 3), (5, 7)      # a pixel of the visible patch, a background pixel
RAY_KINDS = ["dir_nan", "origin_nan", "dir_plus_inf", "dir_minus_inf", "dir_cancels_eps", "dir_cancels_eps_origin_on_plane"]
DEPTH_KINDS = {"depth_nan": float("nan"), "depth_plus_inf": float("inf"), "depth_minus_inf": -float("inf"), "depth_zero": 0.0,
               "depth_minus_zero": -0.0, "depth_negative": -0.5}
# the undilated, uninverted visibility the reference gives the poisoned patch pixel: only d == -1e-6f with the origin off the plane keeps
# the ray (that axis then spans -inf .. +inf and does not constrain it).  The background pixel is invisible in every case.
VISIBLE_AT_P_IN = {k: k == "dir_cancels_eps" for k in RAY_KINDS + list(DEPTH_KINDS)}


def _poisoned(kind):
    o, d, depth, _ = _aabb_scene(HC, WC, place=False)
    for y, x in (P_IN, P_BG):
        if kind == "dir_nan":
            d[y, x, 1] = float("nan")
        elif kind == "origin_nan":
            o[y, x, 1] = float("nan")
        elif kind == "dir_plus_inf":
            d[y, x, 0] = float("inf")
        elif kind == "dir_minus_inf":
            d[y, x, 0] = -float("inf")
        elif kind.startswith("dir_cancels_eps"):      # d + 1e-6 == 0 in fp32: the inverse is +inf.  The camera's z is inside the box's z slab
            d[y, x, 2] = -1e-6
            assert float(d[y, x, 2] + 1e-6) == 0.0 and float(AABB[0, 2]) < float(o[y, x, 2]) < float(AABB[1, 2])
            if kind.endswith("origin_on_plane"):      # ... and on the plane itself the distance is 0 * inf
                o[y, x, 2] = AABB[0, 2]
        else:
            depth[y, x] = DEPTH_KINDS[kind]
    return o, d, depth


def test_poison_pixels_are_where_they_matter():
    """With clean rays the patch pixel is visible and the background pixel is not, and
    their rays hit the box: dropping a NaN axis therefore CHANGES the answer at the patch pixel."""
    o, d, depth, _ = _aabb_scene(HC, WC, place=False)
    vis, _ = su.aabb_mask_and_condition(depth, o, d, AABB, None)
    nears, fars = su.intersect_with_aabb(o, d, AABB)
    assert bool(vis[P_IN]) and not bool(vis[P_BG]) and bool(nears[P_IN] < fars[P_IN]) and bool(nears[P_IN] > 0)
    assert 0.005 < float(vis.float().mean()) < 0.5


@pytest.mark.parametrize("dil", [None, (7, 7)])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("kind", RAY_KINDS + list(DEPTH_KINDS))
def test_non_finite_inputs_match_oracle(gpu, kind, inverse, dil):
    o, d, depth = _poisoned(kind)
    md, color = _combined_extras(HC, WC)
    vis_in = VISIBLE_AT_P_IN[kind] != inverse
    results = []
    for mode, extras in (("aabb", []), ("combined", [md, color])):
        mask, cond = _gpu_call(mode, gpu, [depth, o, d], AABB, extras, dil, inverse)
        rmask, rcond = _oracle(mode, [depth, o, d], AABB, extras, dil, inverse)
        rvis, _ = _oracle(mode, [depth, o, d], AABB, extras, None, inverse)
        results.append((mode, mask.cpu(), cond.cpu(), rmask, rcond, rvis))
        print(f"\n[C] {mode:8s} {kind}, inverse {inverse}, element {dil}: mask mismatches {int((mask.cpu() != rmask).sum())}, condition words "
              f"that differ {_diff_bits(cond, rcond)}; at the patch pixel mask {int(mask[P_IN])} / oracle {int(rmask[P_IN])} (undilated "
              f"{int(rvis[P_IN])}, expected {int(vis_in)}), condition {float(cond[P_IN]):.6g} / {float(rcond[P_IN]):.6g}; at the background pixel "
              f"mask {int(mask[P_BG])} / {int(rmask[P_BG])}, condition {float(cond[P_BG]):.6g} / {float(rcond[P_BG]):.6g}")
    for mode, mask, cond, rmask, rcond, rvis in results:
        # the oracle itself reaches the case: the poisoned pixels come out as derived above
        assert bool(rvis[P_IN]) == vis_in and bool(rvis[P_BG]) == inverse, mode
        for p in (P_IN, P_BG):      # each poisoned pixel on its own
            assert bool(mask[p]) == bool(rmask[p]), (mode, p)
            assert _diff_bits(cond[p], rcond[p]) == 0, (mode, p)
            if dil is None:
                assert bool(mask[p]) == (vis_in if p == P_IN else inverse), (mode, p)
            if kind == "depth_nan":
                assert bool(torch.isnan(cond[p])), (mode, p)      # (NaN - dmin) / range, and 0 * NaN in the combined blend
        assert torch.equal(mask, rmask), mode
        assert _diff_bits(cond, rcond) == 0, mode
    assert torch.equal(results[0][1], results[1][1])      # the combined mode's mask is the aabb mode's


@pytest.mark.parametrize("kind", RAY_KINDS)
def test_intersect_with_aabb_non_finite_rays_match_oracle(gpu, kind):
    o, d, _ = _poisoned(kind)
    nears, fars = intersect_with_aabb(o.to(gpu), d.to(gpu), AABB)
    rn, rf = su.intersect_with_aabb(o, d, AABB)
    nears, fars = nears.cpu(), fars.cpu()
    print(f"\n[C] sn_intersect_with_aabb {kind}: nears words that differ {_diff_bits(nears, rn)}, fars {_diff_bits(fars, rf)}; at the patch pixel "
          f"nears {float(nears[P_IN]):.6g} / oracle {float(rn[P_IN]):.6g}, fars {float(fars[P_IN]):.6g} / {float(rf[P_IN]):.6g}; at the background "
          f"pixel nears {float(nears[P_BG]):.6g} / {float(rn[P_BG]):.6g}, fars {float(fars[P_BG]):.6g} / {float(rf[P_BG]):.6g}")
    want_nan = kind in ("dir_nan", "origin_nan", "dir_cancels_eps_origin_on_plane")
    for p in (P_IN, P_BG):
        assert bool(torch.isnan(rn[p])) == want_nan and bool(torch.isnan(rf[p])) == want_nan, p      # the oracle reaches the case
        assert _diff_bits(nears[p], rn[p]) == 0 and _diff_bits(fars[p], rf[p]) == 0, p
    assert _diff_bits(nears, rn) == 0 and _diff_bits(fars, rf) == 0
