"""The frame plan (signerf_amd/csrc/sn_frame.h), without a GPU: where the fused kernels write in the caller's workspace, the size
sn_workspace_bytes promises, the launch grids and the split-depth tail.  tests/golden/frame_plans.json was recorded by
tests/golden/record_frame_plans.py from the library of the commit that still computed all of it inside sn_api.hip (`provenance`), its HIP
runtime calls served by tests/golden/hip_host_stub.c.
  * the tree's library, driven by the same recorder, must reproduce the file exactly;
  * tests/c/frame_plan.cpp, built with g++ from sn_frame.h and nothing else of the library, must print the recorded values for every case
    (`table`), which ties the header to the reference library without going through the tree's;
  * its `enumerate` mode asserts the plan's invariants over frames x sample counts x proposal iterations x CU counts, and a second build
    with -fsanitize=address,undefined must print the same without a report."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from helpers import GOLDEN, ROOT

RECORDER = os.path.join(GOLDEN, "record_frame_plans.py")
SRC = os.path.join(ROOT, "tests", "c", "frame_plan.cpp")


def _build(tmp, name, flags):
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path, r = _build(str(tmp_path_factory.mktemp("frame_plan")), "frame_plan", [])
    assert r.returncode == 0, r.stderr[-3000:]
    return path


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLDEN, "frame_plans.json")))


def _launch(gold, launches, kernel):
    hits = [l for l in launches if kernel in gold["kernels"][l["kernel"]]]
    assert len(hits) <= 1
    return hits[0] if hits else None


def test_golden_file_names_its_source_and_reaches_every_return_of_plan_tail(gold):
    assert len(gold["provenance"]["parent_commit"]) == 40     # recorded from that commit's library, never from this tree's
    assert "hip_host_stub.c" in gold["provenance"]["procedure"]
    spec = importlib.util.spec_from_file_location("record_frame_plans", RECORDER)
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)      # (the matrix the file was recorded with; nothing runs on import)
    keys = ("name", "height", "width", "S", "cus", "chunk_rays", "nprop", "prec")
    assert [{k: c[k] for k in keys} for c in gold["cases"]] == rec.CASES
    seg = {}      # (height, width, S, cus) -> (seg_first_block, n_seg, seg_len) of the main kernel
    for c in gold["cases"]:
        m = _launch(gold, c["calls"]["rays"], "sn_render_main_kernel")
        seg[(c["height"], c["width"], c["S"], c["cus"])] = (m["seg_first_block"], m["n_seg"], m["seg_len"])
        assert (_launch(gold, c["calls"]["rays"], "sn_main_combine_kernel") is not None) == (m["n_seg"] > 1)
    whole = lambda h, w, S, cus, wgs: seg[(h, w, S, cus)] == (wgs, 1, S)
    assert whole(64, 64, 7, 256, 16)                                         # S < 8
    assert whole(384, 512, 48, 256, 768)                                     # empty tail
    assert whole(200, 200, 48, 256, 169) and whole(800, 800, 48, 256, 2500)  # tail above slots / 8
    assert whole(128, 144, 9, 256, 72)                                       # not worth a second kernel
    assert whole(385, 512, 48, 250, 800)                                     # first_block % 8 != 0
    assert [seg[(64, 64, S, 256)] for S in (8, 16, 48, 64, 256)] == [(0, 2, 4), (0, 2, 8), (0, 4, 12), (0, 5, 13), (0, 8, 32)]
    assert seg[(640, 640, 48, 256)] == (1536, 4, 12) and seg[(800, 800, 48, 64)] == (2496, 4, 12)      # split behind full rounds
    assert {c["nprop"] for c in gold["cases"]} == {0, 1, 2}
    assert any(c["height"] * c["width"] % c["chunk_rays"] for c in gold["cases"])


def test_the_library_reproduces_the_recorded_plans(built_lib, gold, tmp_path):
    """The same matrix through the tree's library, in a child process (the stub must be the first HIP runtime the process loads)."""
    out = str(tmp_path / "tree.json")
    r = subprocess.run([sys.executable, RECORDER, built_lib, "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    tree = json.load(open(out))
    assert tree["kernels"] == gold["kernels"]
    for t, g in zip(tree["cases"], gold["cases"]):
        assert t == g, g["name"]
    assert len(tree["cases"]) == len(gold["cases"])


def test_the_header_alone_prints_the_recorded_plans(exe, gold, tmp_path):
    def opt(v):
        return "None" if v is None else str(v)

    lines, want = [], []
    for c in gold["cases"]:
        eff_main, eff_normals = c["effective_precision"]
        lines.append(" ".join(str(v) for v in (c["height"], c["width"], c["S"], c["nprop"], c["chunk_rays"], c["cus"], int(eff_main == 2), int(eff_normals == 1))))
        plain, expd, normals = (c["calls"][k] for k in ("rays", "rays_expected_depth", "normals"))
        prop, main, combine = (_launch(gold, expd, k) for k in ("sn_proposal_kernel", "sn_render_main_kernel", "sn_main_combine_kernel"))
        nrm = _launch(gold, normals, "sn_normals_kernel")
        # the call without expected_depth and the proposal launch of the normals render plan the same, less the two expected-depth regions
        assert _launch(gold, plain, "sn_render_main_kernel") == dict(main, exp_raw=None, chunk_minmax=None) and _launch(gold, normals, "sn_proposal_kernel") == prop
        assert main["block"] == nrm["block"] == [256, 1, 1] and all(l["grid"][1:] == [1, 1] for l in plain + expd + normals)
        tiles = [main[k] for k in ("tile_w_log2", "tile_h_log2", "tiles_x", "tiles_y")]
        assert all([l[k] for k in ("tile_w_log2", "tile_h_log2", "tiles_x", "tiles_y")] == tiles for l in (prop, nrm, combine) if l)
        assert nrm["ebins"] == main["ebins"]
        w = f"ws={c['workspace_bytes']} prop="
        w += "None" if prop is None else ",".join(opt(v) for v in (prop["grid"][0], prop["block"][0], prop["ebins_out"], prop["scratch"], prop["tile_counter"]))
        w += " main=" + ",".join(opt(v) for v in (main["grid"][0], main["lds"], main["ebins"], main["exp_raw"], main["chunk_minmax"], main["seg_scratch"],
                                                  main["n_chunks"], main["seg_first_block"], main["n_seg"], main["seg_len"]))
        w += " combine=" + ("None" if combine is None else f"{combine['grid'][0]},{combine['lds']}")
        w += f" normals={nrm['grid'][0]},{nrm['lds']} tiles=" + ",".join(map(str, tiles))
        want.append(w)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "table", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want) > 40
    for c, g, w in zip(gold["cases"], got, want):
        assert g == w, c["name"]


def _counts(stdout):
    words = stdout.split()
    return dict(zip(words[0::2], map(int, words[1::2])))


def test_enumeration_holds_the_invariants(exe):
    r = subprocess.run([exe, "enumerate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    n = _counts(r.stdout)
    assert n["plans"] > 5_000_000 and 0 < n["split"] < n["plans"] and n["behind_full_rounds"] > 0 and n["tile_queue"] > 0
    # every way a small tail is left whole occurs in the domain -- the "not worth a second kernel" return too
    assert n["left_whole_no_rows_of_8"] > 0 and n["left_whole_not_worth"] > 0


def test_enumeration_under_address_and_undefined_behaviour_sanitizers(exe, tmp_path):
    san, r = _build(str(tmp_path), "frame_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and any(w in r.stderr for w in ("libasan", "libubsan", "-lasan", "-lubsan", "fsanitize")):
        pytest.skip("this toolchain has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-3000:]
    plain = subprocess.run([exe, "enumerate"], capture_output=True, text=True, timeout=120)
    checked = subprocess.run([san, "enumerate"], capture_output=True, text=True, timeout=300)
    assert checked.returncode == 0 and checked.stderr == "", checked.stderr[-3000:]
    assert checked.stdout == plain.stdout
