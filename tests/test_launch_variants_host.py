"""What the three launch sites of signerf_amd/csrc/sn_api.hip launch, without a GPU: tests/golden/record_launch_variants.py drives the tree's
own library, its HIP runtime calls served by tests/golden/hip_host_stub.c, through the matrix of handles and calls it recorded
tests/golden/launch_variants.json with -- from the library of the commit that still decided inside the launch sites (`provenance`).  Every
call must agree in return code, sn_last_error and the ordered kernels it launches; the digests over grid, block, LDS bytes and parameter
block (pointers as arena offsets) of the launches must agree per handle, entry point, frame and precision; so must what
sn_effective_precision answers and what the handles' layouts say.

One difference is the point of the selectors and is asserted, not tolerated: a call the reference REFUSED after it had already enqueued the
proposal kernel (61 calls: single fp16 or the main-kernel dump on a variant that has none) must now enqueue nothing.

The lists of sn_variant.h are held against the code object too: the names they spell are exactly the instantiations of the three kernels
the tree's library contains."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from helpers import GOLDEN, ROOT

RECORDER = os.path.join(GOLDEN, "record_launch_variants.py")
FUSED = ("sn_render_main_kernel", "sn_proposal_kernel", "sn_normals_kernel")


def recorder():
    """The recorder as a module: its matrix (HANDLES, calls_of) without its run."""
    spec = importlib.util.spec_from_file_location("record_launch_variants", RECORDER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def outcomes(doc, handle):
    """[(return code, error text, [kernel names])] of a handle's calls, in the order of calls_of."""
    out = []
    for i in doc["handles"][handle]["calls"].split():
        rc, err, *kernels = map(int, doc["outcomes"][int(i)].split())
        out.append((rc, doc["errors"][err], [doc["kernels"][k] for k in kernels]))
    return out


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLDEN, "launch_variants.json")))


@pytest.fixture(scope="module")
def tree(built_lib, tmp_path_factory):
    """The same matrix through the tree's library, in a child process (the stub must be the first HIP runtime the process loads)."""
    out = str(tmp_path_factory.mktemp("launch_variants") / "tree.json")
    r = subprocess.run([sys.executable, RECORDER, built_lib, "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.load(open(out))


def test_golden_file_names_its_source_and_reaches_every_instantiation(gold):
    assert len(gold["provenance"]["parent_commit"]) == 40     # recorded from that commit's library, never from this tree's
    assert "hip_host_stub.c" in gold["provenance"]["procedure"]
    assert gold["never_launched"] == []      # every one of the 70 instantiations is launched by some public call of the matrix
    assert sum(any(f in k for f in FUSED) for k in gold["kernels"]) == 70
    rec = recorder()
    assert list(gold["handles"]) == list(rec.HANDLES)
    for name, h in gold["handles"].items():
        assert len(h["calls"].split()) == len(rec.calls_of(rec.HANDLES[name], h["facts"]["has_pred_normals"])), name


def test_same_handles_and_answers(tree, gold):
    assert list(tree["handles"]) == list(gold["handles"])
    for name, g in gold["handles"].items():
        t = tree["handles"][name]
        assert t["facts"] == g["facts"], name
        assert t["effective_precision"] == g["effective_precision"], name


def test_every_call_launches_what_the_reference_launched(tree, gold):
    rec = recorder()
    wrong, refused_after_enqueue = [], 0
    for name, g in gold["handles"].items():
        keys = [k for k, _ in rec.calls_of(rec.HANDLES[name], g["facts"]["has_pred_normals"])]
        mine, theirs = outcomes(tree, name), outcomes(gold, name)
        assert len(mine) == len(theirs) == len(keys), name
        for key, t, (rc, err, kernels) in zip(keys, mine, theirs):
            if rc != 0 and kernels:     # the reference had enqueued something before it refused
                assert all("sn_proposal_kernel" in k for k in kernels), (name, key)
                refused_after_enqueue += 1
                kernels = []
            if t != (rc, err, kernels):
                wrong.append((name, key, (rc, err, kernels), t))
    assert not wrong, (len(wrong), wrong[:3])
    assert refused_after_enqueue == 61


def test_geometry_and_parameter_blocks_of_the_launches(tree, gold):
    """(A digest that differs names its handle, entry point, frame and precision; the recorder, run on both libraries with the print of
    `launches` it is built from, shows the launch.)"""
    wrong = [(name, group) for name, g in gold["handles"].items() for group, digest in g["launch_digests"].items()
             if tree["handles"][name]["launch_digests"].get(group) != digest]
    assert not wrong, wrong
    assert all(set(tree["handles"][n]["launch_digests"]) == set(g["launch_digests"]) for n, g in gold["handles"].items())


def test_the_lists_are_the_instantiations_in_the_code_object(tree, tmp_path):
    exe = str(tmp_path / "variant_select")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "c", "variant_select.cpp"), "-o", exe], check=True)
    listed = subprocess.run([exe, "lists"], capture_output=True, text=True, check=True).stdout.split()
    built = [k for k in tree["kernels"] + tree["never_launched"] if any(f in k for f in FUSED)]     # (never_launched: from the code object's metadata)
    assert len(listed) == len(set(listed))
    for f, n in zip(FUSED, (42, 8, 20)):
        assert sum(f in k for k in listed) == sum(f in k for k in built) == n, f
    assert sorted(listed) == sorted(built)
