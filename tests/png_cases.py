"""The images of the png_encoder="hip" tests (tests/test_png_codes_host.py, tests/test_gpu_png.py) and the serial host reference encoder
built from tests/c/png_encode.cpp.  Every image is the smallest case at which the part its name tells can go wrong; S is the segment size
(SN_PNG_SEGMENT_BYTES of signerf_amd/csrc/sn_png_codes.h, 16384)."""
import functools
import io
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "c", "png_encode.cpp")
S = 16384
MAX_DIM = 8192


def stream_image(n, rng):
    """A greyscale image whose filtered stream has exactly n bytes, every one but the rows' filter bytes drawn from {0..3} (so matches
    are dense at every segment boundary), with as few rows as the 8192 limit on the width allows: one row up to n = 8193 -- a single
    row cannot reach S = 16384 -- else the fewest that divide n.  The pixels are the column sums mod 256, which filter "Up" undoes."""
    h = next(h for h in range(1, 64) if n % h == 0 and n // h - 1 <= MAX_DIM)
    w = n // h - 1
    d = rng.integers(0, 4, (h, w), dtype=np.uint8)
    return np.cumsum(d, axis=0, dtype=np.uint64).astype(np.uint8).reshape(h, w, 1)


def fibonacci_row(rng):
    """One row whose byte frequencies are Fib(1..18) (6764 pixels): an unlimited Huffman tree over them (and EOB) is deeper than 15."""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    row = np.concatenate([np.full(f, 7 * i + 3, np.uint8) for i, f in enumerate(fib)])
    rng.shuffle(row)
    return row.reshape(1, -1, 1)


def smooth_rgb(h, w):
    """Low-frequency shading like a render's: a few sinusoids per channel, quantised to 8 bits."""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    chan = lambda a, b, c: 127.5 + 80 * np.sin(a * xx / w + b * yy / h) + 45 * np.cos(c * (xx / w) * (yy / h) + a)   # noqa: E731
    return np.stack([chan(3.1, 4.3, 5.9), chan(5.3, 2.2, 3.7), chan(2.4, 6.1, 4.8)], -1).astype(np.uint8)


def disc_mask(n):
    yy, xx = np.mgrid[:n, :n]
    return (((yy - n // 2) ** 2 + (xx - n // 2) ** 2 < (3 * n // 8) ** 2) * 255).astype(np.uint8)[..., None]


@functools.lru_cache(maxsize=None)
def images():
    """name -> uint8 [H,W,C] array (read-only)."""
    rng = np.random.default_rng(20240607)
    smooth = smooth_rgb(200, 200)
    cond = smooth_rgb(192, 192) * (disc_mask(192) > 0)     # condition-like: the scene inside the mask, black outside
    big_rgb = (smooth_rgb(1080, 1920) + rng.integers(0, 3, (1080, 1920, 3))).astype(np.uint8)
    yy, xx = np.mgrid[:4100, :4100]
    big_grey = ((yy // 3 + xx // 5) % 256).astype(np.uint8)[..., None]
    out = {
        "1x1x1": np.array([[[7]]], np.uint8),
        "1x1x3": np.array([[[7, 0, 255]]], np.uint8),
        "1x17x3": rng.integers(0, 256, (1, 17, 3), dtype=np.uint8),
        "23x1x1": rng.integers(0, 256, (23, 1, 1), dtype=np.uint8),
        "2x2x3": rng.integers(0, 256, (2, 2, 3), dtype=np.uint8),
        "37x53x3": rng.integers(0, 5, (37, 53, 3), dtype=np.uint8),
        "row_8192": rng.integers(0, 4, (1, 8192, 1), dtype=np.uint8),
        "stream_S-1": stream_image(S - 1, rng),
        "stream_S": stream_image(S, rng),
        "stream_S+1": stream_image(S + 1, rng),
        "stream_2S+1": stream_image(2 * S + 1, rng),
        "zeros_256": np.zeros((256, 256, 1), np.uint8),
        "full_256": np.full((256, 256, 1), 255, np.uint8),
        "noise_200": rng.integers(0, 256, (200, 200, 3), dtype=np.uint8),
        "smooth_200": smooth,
        "smooth_noise_200": (smooth + rng.integers(0, 3, smooth.shape)).astype(np.uint8),
        "disc_192": disc_mask(192),
        "condition_192": cond.astype(np.uint8),
        "fibonacci_row": fibonacci_row(rng),
        "segments_gt_256": big_rgb,
        "segments_gt_1024": big_grey,
    }
    for a in out.values():
        a.setflags(write=False)
    return out


NAMES = ["1x1x1", "1x1x3", "1x17x3", "23x1x1", "2x2x3", "37x53x3", "row_8192", "stream_S-1", "stream_S", "stream_S+1", "stream_2S+1",
         "zeros_256", "full_256", "noise_200", "smooth_200", "smooth_noise_200", "disc_192", "condition_192", "fibonacci_row",
         "segments_gt_256", "segments_gt_1024"]
# file <= factor * len(encode_png(image, 6))
LEVEL6_FACTOR = {"smooth_200": 2.5, "disc_192": 2.5, "condition_192": 2.5, "smooth_noise_200": 1.25}


def filtered_stream(u8):
    """The array `raw` of dataset_io.encode_png, as bytes."""
    h, w, c = u8.shape
    flat = np.ascontiguousarray(u8).reshape(h, w * c)
    raw = np.empty((h, 1 + w * c), dtype=np.uint8)
    raw[0, 0] = 0
    raw[0, 1:] = flat[0]
    if h > 1:
        raw[1:, 0] = 2
        np.subtract(flat[1:], flat[:-1], out=raw[1:, 1:])
    return raw.tobytes()


def chunks(png):
    """[(tag, data)] of a PNG file, every CRC checked."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, p = [], 8
    while p < len(png):
        n, = struct.unpack(">I", png[p:p + 4])
        tag, data = png[p + 4:p + 8], png[p + 8:p + 8 + n]
        assert struct.unpack(">I", png[p + 8 + n:p + 12 + n])[0] == zlib.crc32(tag + data), tag
        out.append((tag, data))
        p += 12 + n
    assert p == len(png)
    return out


def check_file(png, u8):
    """One IDAT holding a 78 01 stream that inflates to the filtered scanlines; Pillow reads the pixels back."""
    from PIL import Image

    h, w, c = u8.shape
    ch = chunks(png)
    assert [t for t, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert ch[1][1][:2] == b"\x78\x01"
    assert zlib.decompress(ch[1][1]) == filtered_stream(u8)
    im = Image.open(io.BytesIO(png))
    im.load()
    assert im.mode == ("L" if c == 1 else "RGB") and im.size == (w, h)
    assert np.array_equal(np.asarray(im).reshape(h, w, c), u8)


def build_reference(out_dir, sanitize=False):
    exe = os.path.join(out_dir, "png_encode_san" if sanitize else "png_encode")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SOURCE, "-o", exe], check=True)
    return exe


def reference_png(exe, u8, mode=None):
    """The host reference encoder's file for an image; its stderr must stay empty (a sanitizer report lands there)."""
    h, w, c = u8.shape
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.raw"), os.path.join(d, "out.png")
        np.ascontiguousarray(u8).tofile(src)
        r = subprocess.run([exe, "encode", str(h), str(w), str(c), src, dst] + ([mode] if mode else []), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        with open(dst, "rb") as f:
            return f.read()
