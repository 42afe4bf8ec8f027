"""The host packers of the weight images (signerf_amd/csrc/sn_weights.h), without a GPU: tests/c/weights_pack.cpp is built from that
header alone with g++, fed the seeded cases of tests/weights_cases.py, and every image it writes is held, by SHA-256, against the digests
tests/golden/weight_images.json records from the library of the commit that still packed inside sn_finalize_weights (read back through
its sn_debug_read; `provenance` and tests/golden/record_weight_images.py say how).  The scalars that commit exposed through the C ABI -- the feature scales and the effective precisions -- are
compared too; s1 .. s4 and the normals' gradient scale were never readable there, they reach the images (biases, the 1 / s2 slot, the
reverse-pass plane), so the digests cover them, and the printed 1 / s2 is checked against the float the image holds.

A second build of the same program with -fsanitize=address,undefined runs every case and must finish without a report."""
import hashlib
import json
import math
import os
import struct
import subprocess

import pytest

import weights_cases as wc
from helpers import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "c", "weights_pack.cpp")
CASES = wc.cases()


@pytest.fixture(scope="session")
def gold():
    """tests/golden/weight_images.json: recorded from the library of the commit before the packers moved, never from this tree."""
    path = os.path.join(GOLDEN, "weight_images.json")
    assert os.path.exists(path), "tests/golden/weight_images.json is missing: tests/golden/record_weight_images.py records it from the reference commit's library"
    return json.load(open(path))


def _build(tmp, name, flags):
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], capture_output=True, text=True)
    return exe, r


def run_case(exe, case, out_dir):
    """Runs the program on one case: (its scalar line as a dict, {image: bytes})."""
    os.makedirs(out_dir, exist_ok=True)
    inp = os.path.join(out_dir, "input.bin")
    case.input_file().astype("<f4").tofile(inp)
    r = subprocess.run([exe, inp, out_dir], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (case.name, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout), {im: open(os.path.join(out_dir, im + ".bin"), "rb").read() for im in case.images()}


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """Every case through the plain build, once for the module."""
    tmp = str(tmp_path_factory.mktemp("weights_pack"))
    exe, r = _build(tmp, "weights_pack", [])
    assert r.returncode == 0, r.stderr[-3000:]
    return {name: run_case(exe, case, os.path.join(tmp, name)) for name, case in CASES.items()}


def test_golden_file_covers_the_cases_and_names_its_source(gold):
    assert set(gold["cases"]) == set(CASES)
    assert len(gold["provenance"]["parent_commit"]) == 40 and "sn_debug_read" in gold["provenance"]["procedure"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_images_match_the_bytes_the_reference_library_held(packed, gold, name):
    scal, images = packed[name]
    gold, case = gold["cases"][name], CASES[name]
    assert set(images) == set(gold["sha256"]) == set(case.images())
    for im, blob in images.items():
        assert len(blob) == wc.IMAGE_BYTES[im] == scal["sizes"]["prop" if im.startswith("prop") else im]
        assert hashlib.sha256(blob).hexdigest() == gold["sha256"][im], (name, im)
    # the scalars the handle keeps: feature scales, and what a split-precision request resolves to for the render / normals kernels
    assert [scal["t0"]] + scal["t0p"] == gold["feature_scale"]
    assert [scal["split_ok"], scal["normals_split_ok"]] == gold["precision"]
    assert scal["has_pred_normals"] == int(case.pred_normals)
    # 1 / s2 as the split-precision image carries it (SnMainImgH: fp32 tail at byte 40960, B3 + 3 = float 419 of the tail)
    inv_s2, = struct.unpack_from("<f", images["main_h"], 40960 + 4 * 419)
    assert inv_s2 == 1.0 / scal["s2"]
    for k in ("t0", "s1", "s2", "s3", "s4", "grad_scale_normals"):      # powers of two, inside pow2_floor's clamp
        m, e = math.frexp(scal[k])
        assert m == 0.5 and -79 <= e <= 81, (k, scal[k])


def test_branches_the_cases_were_chosen_for(packed):
    s = {n: packed[n][0] for n in CASES}
    assert s["ordinary"]["split_ok"] == 1 and s["ordinary"]["split_why"] == "" and s["ordinary"]["t0"] == 2.0 ** 19
    assert s["bare"]["has_pred_normals"] == 0 and len(s["bare"]["t0p"]) == 1
    assert s["small_table"]["t0"] == 2.0 ** 23
    assert s["density_weight_leaves_fp16"]["split_ok"] == 0 and "leaves the fp16 range" in s["density_weight_leaves_fp16"]["split_why"]
    assert s["table_not_finite"]["split_ok"] == 0 and s["table_not_finite"]["split_why"] == "the hash table holds non-finite values"
    assert s["table_not_finite"]["t0p"] == [2.0 ** 19, 1.0]             # (its second proposal table is not finite either)
    assert s["bias_infinite"]["split_ok"] == 0 and s["bias_infinite"]["split_why"] == "non-finite MLP parameters"
    assert s["proposal_leaves_fp16"]["t0p"] == [2.0 ** 19, 1.0]
    z = s["zero_table_zero_wc3"]
    assert z["t0"] == 1.0 and z["t0p"] == [1.0, 1.0]
    inv_s5, = struct.unpack_from("<f", packed["zero_table_zero_wc3"][1]["main_h"], 42640 + 4096)    # SnMainImgF16::TAILF
    assert inv_s5 == 1.0


def test_every_case_under_address_and_undefined_behaviour_sanitizers(packed, tmp_path):
    exe, r = _build(str(tmp_path), "weights_pack_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and any(w in r.stderr for w in ("libasan", "libubsan", "-lasan", "-lubsan", "fsanitize")):
        pytest.skip("this toolchain has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-3000:]
    for name, case in CASES.items():
        scal, images = run_case(exe, case, str(tmp_path / name))       # (asserts exit status 0 and an empty stderr: no report)
        assert scal == packed[name][0] and images == packed[name][1], name
