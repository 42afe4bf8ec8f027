"""The launch selectors (signerf_amd/csrc/sn_variant.h), without a GPU and without the library: tests/c/variant_select.cpp is built from
that header alone with g++.  It enumerates the product of handle facts x requests -- every selection must be in the list of built
instantiations, every refusal must carry its code and a text -- and it is fed every call of tests/golden/launch_variants.json whose outcome
the selectors decide (what the reference library launched or refused for it, recorded from the commit before the selectors existed): the
tuple it selects must spell the recorded kernel names, a refusal the recorded text.

A second build of the same program with -fsanitize=address,undefined runs the enumeration and must finish without a report."""
import importlib.util
import json
import os
import subprocess

import pytest

from helpers import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "c", "variant_select.cpp")
FUSED = ("sn_render_main_kernel", "sn_proposal_kernel", "sn_normals_kernel")
ENTRY = {"r": 0, "d": 1, "n": 2}
FAR = {"far": "1000", "far2e7": "2e7", "farnan": "nan"}


def _build(tmp, name, flags):
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path, r = _build(str(tmp_path_factory.mktemp("variant_select")), "variant_select", [])
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def recorded_lines(gold):
    """One line of `variant_select check` per recorded call the selectors decide: not the calls valid_opts or the argument checks stop
    (their texts begin with the entry point's name), not the SN_ERR_STATE ones (reuse_final_bins, the missing predicted-normals head)."""
    spec = importlib.util.spec_from_file_location("record_launch_variants", os.path.join(GOLDEN, "record_launch_variants.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)      # (the matrix the file was recorded with: HANDLES, calls_of; nothing runs on import)
    lines = []
    for name, h in gold["handles"].items():
        f = h["facts"]
        props = f["prop_scalings"] + [[0.0] * 5] * (2 - len(f["prop_scalings"]))
        head = [f["main_grid_mode"], f["prop_grid_mode"], f["log2_hashmap_size"], f["num_proposals"], f["nd_torch"], *(f["nd_prop"] + [0, 0])[:2], f["split_ok"],
                f["normals_split_ok"], f["has_half_grid"], f["has_dense_main"], f["box"], *f["main_scalings"], *props[0], *props[1]]
        calls = rec.calls_of(rec.HANDLES[name], f["has_pred_normals"])
        assert len(calls) == len(h["calls"].split())
        for (_, c), o in zip(calls, h["calls"].split()):
            rc, err, *kernels = map(int, gold["outcomes"][int(o)].split())
            text = gold["errors"][err]
            if rc == 3 or text.startswith(("sn_render_rays: ", "sn_render_normals: ")):
                continue
            call = [ENTRY[c["entry"]], c["nprop"], c["prec"], c["spacing"], FAR[c["far"]], c["march"], c["reuse"]]
            names = [gold["kernels"][k] for k in kernels]
            picked = [next((n for n in names if k in n), "-") for k in FUSED]
            lines.append("\t".join([" ".join(str(v) for v in head + call), picked[0], picked[1], picked[2], text]))
    return lines


def test_enumeration_selects_only_what_is_built(exe):
    r = subprocess.run([exe, "enumerate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    counts = dict(zip(r.stdout.split()[0:6:2], map(int, r.stdout.split()[1:6:2])))
    assert counts["combinations"] > 20000 and 0 < counts["refused"] < counts["combinations"] - counts["invalid"]
    assert "never selected" not in r.stdout     # every listed instantiation is selected by some combination


def test_selectors_spell_what_the_reference_library_launched(exe, tmp_path):
    gold = json.load(open(os.path.join(GOLDEN, "launch_variants.json")))
    lines = recorded_lines(gold)
    assert len(lines) > 4000 and sum(1 for ln in lines if ln.endswith("\t")) > 1000 and sum(1 for ln in lines if not ln.endswith("\t")) > 1000
    path = tmp_path / "recorded.tsv"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "check", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.split() == ["checked", str(len(lines))]


def test_enumeration_under_address_and_undefined_behaviour_sanitizers(exe, tmp_path):
    san, r = _build(str(tmp_path), "variant_select_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and any(w in r.stderr for w in ("libasan", "libubsan", "-lasan", "-lubsan", "fsanitize")):
        pytest.skip("this toolchain has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-3000:]
    plain = subprocess.run([exe, "enumerate"], capture_output=True, text=True, timeout=120)
    checked = subprocess.run([san, "enumerate"], capture_output=True, text=True, timeout=300)
    assert checked.returncode == 0 and checked.stderr == "", checked.stderr[-3000:]
    assert checked.stdout == plain.stdout
