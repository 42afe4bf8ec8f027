"""What the entry points that take no SnHandle refuse and launch, without a GPU: tests/golden/record_handle_free.py drives the tree's own
library, its HIP runtime calls served by tests/golden/hip_host_stub.c, through the matrix of calls it recorded
tests/golden/handle_free_launches.json with -- from the library of the commit that still had all of them in sn_api.hip (`provenance`).
Every call must agree in return code, sn_last_error text, the ordered kernels with grid, block and LDS bytes, the digest of the parameter
block of every launch (pointers as arena offsets) and, for the mask steps, the statistics words of the workspace; the size and version
queries must give what that commit's gave.  (Where a digest differs, the recorder run on both libraries with block.hex() printed shows
the bytes.)"""
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest

from helpers import GOLDEN, ROOT

RECORDER = os.path.join(GOLDEN, "record_handle_free.py")


def recorder():
    """The recorder as a module: its matrix (CALLS, QUERIES) without its run."""
    spec = importlib.util.spec_from_file_location("record_handle_free", RECORDER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLDEN, "handle_free_launches.json")))


@pytest.fixture(scope="module")
def tree(built_lib, tmp_path_factory):
    """The same matrix through the tree's library, in a child process (the stub must be the first HIP runtime the process loads)."""
    out = str(tmp_path_factory.mktemp("handle_free") / "tree.json")
    r = subprocess.run([sys.executable, RECORDER, built_lib, "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.load(open(out))


def test_golden_file_names_its_source_and_its_matrix(gold):
    rec = recorder()
    assert len(gold["provenance"]["parent_commit"]) == 40 and gold["provenance"]["parent_commit"] == rec.PARENT      # never recorded from this tree
    assert "hip_host_stub.c" in gold["provenance"]["procedure"]
    assert [c["key"] for c in gold["calls"]] == [key for key, *_ in rec.CALLS]
    assert [q[:2] for q in gold["queries"]] == [[fn, list(a)] for fn, a in rec.QUERIES]
    assert sorted(s[0] for s in gold["stamps"]) == sorted(rec.STAMPS)
    assert sum(c["rc"] == 0 for c in gold["calls"]) >= 90 and sum(c["rc"] != 0 for c in gold["calls"]) >= 200


def test_every_handle_free_entry_point_is_in_the_matrix():
    """Every function of _lib's recorded headers whose prototype names no SnHandle: called by the matrix, or -- the *_abi_version and
    *_bytes queries -- by QUERIES."""
    from signerf_amd import _lib

    rec = recorder()
    headers = "".join(open(os.path.join(ROOT, "include", h)).read() for h in sorted(os.listdir(os.path.join(ROOT, "include"))))
    names = list(_lib.functions(recorded=True))      # (no name twice: tests/test_cabi.py, over the whole registry)
    assert len(names) > 50
    called, queried = {fn for _, fn, *_ in rec.CALLS}, {fn for fn, _ in rec.QUERIES}
    free = []
    for n in names:
        proto = re.search(r"^[A-Za-z_][\w \*]*\b" + n + r"\s*\(([^;{]*)\)\s*;", headers, re.M)      # (a declaration, not a comment's mention)
        assert proto, n
        if "SnHandle" not in proto.group(1):
            free.append(n)
            is_query = n.endswith("_abi_version") or n.endswith("_bytes")
            assert n in (queried if is_query else called), n
    assert len(free) == len(called) + len(queried) and not called & queried


def test_queries_answer_what_the_reference_answered(tree, gold):
    assert tree["queries"] == gold["queries"]


def test_the_same_calls_clear_a_workspace_stamp(tree, gold):
    """An accepted mask step or raster clears the stamp of its workspace (reuse_final_bins is then refused), one refused before it
    touched the workspace does not, and the PNG encoder never does."""
    assert tree["stamps"] == gold["stamps"]
    assert {s[2] for s in gold["stamps"] if s[1] == 0 and "png" not in s[0]} == {3} and {s[2] for s in gold["stamps"] if s[1] != 0} == {0}


def test_every_call_is_refused_or_launched_as_the_reference_did(tree, gold):
    assert tree["kernels"] == gold["kernels"]
    assert len(tree["calls"]) == len(gold["calls"])
    wrong = [(g, t) for g, t in zip(gold["calls"], tree["calls"]) if g != t]
    assert not wrong, (len(wrong), [(g["key"], g["rc"], g["error"], t["rc"], t["error"]) for g, t in wrong[:5]])
