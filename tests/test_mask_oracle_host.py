"""The structuring element seen on its own, CPU side.  A single set pixel, dilated, is the element reflected about its anchor:
set pixel (py, px), element ``E`` [kh, kw], anchor (kh // 2, kw // 2) -> ``dst[py - (i - ay), px - (j - ax)]`` for every set ``E[i, j]``.
``impulse_response`` builds that image (for several set pixels: the union, clipped at the border) from ``ellipse_element`` alone, without
the oracle's ``dilate`` -- whose loop over the element's pixels is too slow for 256x256 elements.  This file pins that the construction IS
``su.dilate`` wherever both can be afforded; tests/test_gpu_mask_edges.py then holds the HIP dilation against it for every element size.
"""
import numpy as np
import pytest

from oracle import signerf_utils as su


def impulse_response(H, W, points, elem):
    """uint8 [H, W]: the dilation by `elem` (anchor = centre, nothing outside the image contributes) of the image whose set pixels are
    `points` [(py, px), ...] -- the union of the element's reflections, one per point, clipped to the image."""
    kh, kw = elem.shape
    ay, ax = kh // 2, kw // 2
    refl = np.ascontiguousarray(elem[::-1, ::-1]) != 0   # refl[i', j'] = elem[kh - 1 - i', kw - 1 - j']
    out = np.zeros((H, W), dtype=bool)
    for py, px in points:
        top, left = py - (kh - 1 - ay), px - (kw - 1 - ax)   # where refl[0, 0] lands
        y0, y1, x0, x1 = max(top, 0), min(top + kh, H), max(left, 0), min(left + kw, W)
        if y0 < y1 and x0 < x1:
            out[y0:y1, x0:x1] |= refl[y0 - top : y1 - top, x0 - left : x1 - left]
    return out.astype(np.uint8)


def border_points(H, W):
    """The four corners and the four edge midpoints of an H x W image (coinciding ones once)."""
    ys, xs = (0, (H - 1) // 2, H - 1), (0, (W - 1) // 2, W - 1)
    return sorted({(y, x) for y in ys for x in xs} - {(ys[1], xs[1])} if H > 2 and W > 2 else {(y, x) for y in ys for x in xs})


def _image(H, W, points):
    src = np.zeros((H, W), dtype=float)
    for py, px in points:
        src[py, px] = 1.0
    return src


SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 17, 21, 31, 32, 33, 50, 63, 64]   # 22 x 22 = 484 (w, h) pairs


@pytest.mark.parametrize("w", SIZES)
def test_impulse_response_is_the_oracles_dilate(w):
    """Every (w, h) of SIZES x SIZES: a centred impulse in a (2h+3) x (2w+3) image (nothing clips), then the corners and edge midpoints of an
    image smaller than the element (every side clips)."""
    n = 0
    for h in SIZES:
        elem = su.ellipse_element(w, h)
        assert elem.shape == (h, w) and elem.any()
        H, W = 2 * h + 3, 2 * w + 3
        pts = [(h + 1, w + 1)]
        want = su.dilate(_image(H, W, pts), elem) > 0
        got = impulse_response(H, W, pts, elem)
        assert np.array_equal(got != 0, want), (w, h)
        assert int(got.sum()) == int(elem.sum())          # nothing clipped, nothing lost
        Hs, Ws = max(1, h // 2), max(1, w // 2)
        pts = border_points(Hs, Ws)
        want = su.dilate(_image(Hs, Ws, pts), elem) > 0
        assert np.array_equal(impulse_response(Hs, Ws, pts, elem) != 0, want), (w, h, "clipped")
        n += 1
    print(f"element width {w}: {n} heights, centred and clipped impulse responses equal su.dilate")
    assert n == len(SIZES)


def test_impulse_response_shows_a_missing_reflection():
    """The construction can tell a reflected element from an unreflected one exactly when the element is not point-symmetric about its
    anchor: every element with an even side.  (An odd x odd ellipse is symmetric, so only even sizes observe the reflection.)"""
    for w, h, symmetric in ((5, 5, True), (9, 5, True), (4, 4, False), (2, 2, False), (6, 5, False), (5, 6, False), (50, 50, False)):
        elem = su.ellipse_element(w, h)
        H, W = 2 * h + 3, 2 * w + 3
        got = impulse_response(H, W, [(h + 1, w + 1)], elem)
        plain = np.zeros((H, W), dtype=np.uint8)           # the element pasted WITHOUT the reflection, anchor on the impulse
        plain[h + 1 - h // 2 : h + 1 - h // 2 + h, w + 1 - w // 2 : w + 1 - w // 2 + w] = elem
        assert np.array_equal(got, plain) == symmetric, (w, h)


def test_degenerate_elements():
    """1 x N and N x 1 (r == 0 or c == 0), 2 x 2 and 1 x 1, written out."""
    assert su.ellipse_element(1, 1).tolist() == [[1]]
    assert su.ellipse_element(5, 1).tolist() == [[0, 0, 1, 0, 0]]           # r == 0: dx = round(c * sqrt(0 * 0)) = 0, the centre column alone
    assert su.ellipse_element(1, 5).tolist() == [[1]] * 5                     # c == 0: one column, every row with |dy| <= r
    assert su.ellipse_element(1, 4).tolist() == [[1]] * 4
    assert su.ellipse_element(2, 2).tolist() == [[0, 1], [1, 1]]
    got = impulse_response(5, 5, [(2, 2)], su.ellipse_element(2, 2))          # reflected about anchor (1, 1): (2,2) -> (2,2), (2,3)... mirrored
    assert got.tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 1, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]
    assert np.array_equal(got != 0, su.dilate(_image(5, 5, [(2, 2)]), su.ellipse_element(2, 2)) > 0)
