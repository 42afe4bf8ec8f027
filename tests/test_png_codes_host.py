"""png_encoder="hip", CPU side: signerf_amd/csrc/sn_png_codes.h -- the header that decides every byte of such a file -- through the serial
reference encoder tests/c/png_encode.cpp, a stand-alone program built twice: plain and with -fsanitize=address,undefined (no preload is
involved).  Both builds must print and write the same and report nothing.  Then the companion C header include/signerf_hip_png.h against
the binding and the library's exports, and the refusals of ``sn_png_encode`` (in a child process: nothing is launched).  No GPU."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import png_cases as pc
from abi_helpers import refusal_sweep
from helpers import ROOT
from signerf_amd import _lib, dataset_io

HEADER = os.path.join(ROOT, "include", "signerf_hip_png.h")


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("png_encode"))
    return pc.build_reference(d), pc.build_reference(d, sanitize=True)


def both(builds, *args):
    outs = []
    for exe in builds:
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (exe, args[:3], r.returncode, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    return outs[0]


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


@pytest.mark.parametrize("name,counts,used", [
    ("fibonacci_24", fib(24), 24),                                   # an unlimited tree is 23 deep
    ("fibonacci_24_in_286", [0] * 100 + fib(24) + [0] * 162, 24),
    ("one_symbol", [0] * 256 + [1] + [0] * 29, 2),                  # a second symbol joins: the code must be complete
    ("one_symbol_is_0", [5] + [0] * 29, 2),
    ("two_symbols", [0, 9, 0, 0, 1], 2),
    ("all_286_differ", [1 + (i * 37) % 1000 for i in range(286)], 286),
    ("all_equal_286", [7] * 286, 286),
    ("all_equal_30", [3] * 30, 30),
])
def test_code_lengths_are_limited_and_complete(builds, name, counts, used):
    out = both(builds, "lengths", *counts).splitlines()
    lens = [int(x) for x in out[0].split()]
    deepest, kraft = (int(x) for x in out[1].split())
    assert len(lens) == len(counts) and sum(l > 0 for l in lens) == used
    assert all(l > 0 for l, c in zip(lens, counts) if c > 0)
    assert 1 <= deepest <= 15 and deepest == max(lens)
    assert kraft == 1 << 15                                        # Kraft sum exactly 1
    # a rarer symbol never has the shorter code
    assert all(lens[i] >= lens[j] for i in range(len(counts)) for j in range(len(counts)) if 0 < counts[i] < counts[j])


def test_no_used_symbol_gives_no_code(builds):
    assert both(builds, "lengths", *([0] * 30)).splitlines()[0].split() == ["0"] * 30


def test_checksums_combine_from_three_uneven_pieces(builds, tmp_path):
    rng = np.random.default_rng(5)
    for n, a, b in ((100003, 1, 70001), (70000, 0, 65521), (3, 1, 2), (300000, 299999, 300000)):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes() if n != 70000 else b"\xff" * n
        path = tmp_path / f"sums_{n}.bin"
        path.write_bytes(data)
        crc, adler, adler_sums = (int(x) for x in both(builds, "sums", path, a, b).split())
        assert crc == zlib.crc32(data) and adler == zlib.adler32(data) == adler_sums, (n, a, b)


@pytest.mark.parametrize("name", pc.NAMES)
def test_reference_encoder_files(builds, name):
    u8 = pc.images()[name]
    h, w, c = u8.shape
    png = pc.reference_png(builds[0], u8)
    assert png == pc.reference_png(builds[1], u8)                  # the sanitizer build: same bytes, no report
    assert png == pc.reference_png(builds[1], u8, "bits")          # match lengths from the packed equality bits, as the kernel takes them
    pc.check_file(png, u8)
    seg, nseg, bound, _ = (int(x) for x in both(builds, "plan", h, w, c).split())
    raw = len(pc.filtered_stream(u8))
    assert seg == pc.S and 8 * 1024 <= seg <= 32 * 1024 and nseg == -(-raw // seg) and bound == 63 + raw + 5 * nseg
    assert len(png) <= bound
    if name == "noise_200":
        assert len(png) <= raw + 5 * nseg + 69                     # stored blocks plus framing
    if name in ("zeros_256", "full_256"):
        assert len(png) <= 0.04 * raw
    if name in pc.LEVEL6_FACTOR:
        assert len(png) <= pc.LEVEL6_FACTOR[name] * len(dataset_io.encode_png(u8, 6))


def test_segment_plan_of_the_boundary_and_large_cases(builds):
    """The header's plan for the cases named after their segment counts: more than 256 and more than 1024 segments (a scan in several
    passes), and streams of S - 1, S, S + 1, 2 S + 1 bytes in 1, 1, 2 and 3 segments."""
    im = pc.images()
    nseg = lambda name: int(both(builds, "plan", *im[name].shape).split()[1])   # noqa: E731
    assert nseg("segments_gt_256") > 256 and nseg("segments_gt_1024") > 1024
    assert [len(pc.filtered_stream(im["stream_" + k])) for k in ("S-1", "S", "S+1", "2S+1")] == [pc.S - 1, pc.S, pc.S + 1, 2 * pc.S + 1]
    assert [nseg("stream_" + k) for k in ("S-1", "S", "S+1", "2S+1")] == [1, 1, 2, 3]


def test_refused_shapes_have_no_plan(builds):
    for shape in ((0, 4, 3), (4, 0, 1), (8193, 4, 3), (4, 8193, 1), (4, 4, 2), (4, 4, 4), (-1, 4, 3)):
        assert both(builds, "plan", *shape).split()[1:] == ["0", "0", "0"]


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
def test_png_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    assert sorted(_lib.header("png").functions) == ["sn_png_abi_version", "sn_png_encode", "sn_png_max_file_bytes", "sn_png_segment_bytes",
                                                    "sn_png_workspace_bytes"]
    lib = _lib.load()
    assert lib.sn_png_abi_version() == _lib.header("png").version == 1
    assert lib.sn_png_segment_bytes() == pc.S
    blob = open(built_lib, "rb").read()
    names = set(re.findall(rb"_Z\d+(sn_png_[a-z_]+_kernel)", blob))
    assert names == {b"sn_png_segment_deflate_kernel", b"sn_png_finish_file_kernel", b"sn_png_compact_bytes_kernel"}
    assert all(len(n) > 23 for n in names)       # tests/test_launch_variants_host.py indexes the sorted mangled names


def test_size_queries_follow_the_segment_plan(built_lib, builds):
    lib = _lib.load()
    for shape in ((1, 1, 1), (37, 53, 3), (800, 800, 3), (8192, 8192, 3), (8192, 8192, 1), (0, 4, 3), (4, 8193, 1), (4, 4, 2)):
        _, nseg, bound, ws = (int(x) for x in both(builds, "plan", *shape).split())
        assert (lib.sn_png_max_file_bytes(*shape), lib.sn_png_workspace_bytes(*shape)) == (bound, ws), shape
        assert ws >= nseg * (5 + pc.S)


_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
fake = 0x10000   # never dereferenced: every call below is refused before the device is touched
def call(image=fake, h=20, w=24, c=3, ws=fake, ws_bytes=None, out=fake, cap=None, count=fake):
    ws_bytes = lib.sn_png_workspace_bytes(20, 24, 3) if ws_bytes is None else ws_bytes
    cap = lib.sn_png_max_file_bytes(20, 24, 3) if cap is None else cap
    st = lib.sn_png_encode(image, h, w, c, ws, ws_bytes, out, cap, count, N)
    msg = lib.sn_last_error(None)
    return "%d:%s" % (st, "text" if (msg and b"sn_png_encode" in msg) else "notext")
big = 1 << 40
calls = {
 "null_image": lambda: call(image=N), "null_workspace": lambda: call(ws=N), "null_file": lambda: call(out=N), "null_count": lambda: call(count=N),
 "c_0": lambda: call(c=0, ws_bytes=big, cap=big), "c_2": lambda: call(c=2, ws_bytes=big, cap=big), "c_4": lambda: call(c=4, ws_bytes=big, cap=big),
 "h_0": lambda: call(h=0, ws_bytes=big, cap=big), "h_8193": lambda: call(h=8193, ws_bytes=big, cap=big), "h_negative": lambda: call(h=-3, ws_bytes=big, cap=big),
 "w_0": lambda: call(w=0, ws_bytes=big, cap=big), "w_8193": lambda: call(w=8193, ws_bytes=big, cap=big),
 "workspace_short": lambda: call(ws_bytes=lib.sn_png_workspace_bytes(20, 24, 3) - 1),
 "workspace_misaligned": lambda: call(ws=fake + 4),
 "capacity_short": lambda: call(cap=lib.sn_png_max_file_bytes(20, 24, 3) - 1),
}
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_png_encode_refuses_bad_arguments_before_the_device(built_lib):
    got = refusal_sweep(_SWEEP)
    assert len(got) == 15 and got == {k: "1:text" for k in got}


def test_encoder_option_values(tmp_path):
    assert dataset_io.GeneratedDataset(tmp_path, "a", png_encoder="hip").png_encoder == "hip"      # nothing touches the GPU before a save
    with pytest.raises(ValueError, match="levels"):
        dataset_io.GeneratedDataset(tmp_path, "b", png_encoder="hip", png_compress_level=6)
    with pytest.raises(ValueError, match="png_encoder"):
        dataset_io.GeneratedDataset(tmp_path, "c", png_encoder="gpu")
    with pytest.raises(ValueError, match="GPU"):
        dataset_io.encode_png_hip(np.zeros((4, 4, 3), np.uint8))
    assert "PIL on the host, as in the reference" not in dataset_io.__doc__
