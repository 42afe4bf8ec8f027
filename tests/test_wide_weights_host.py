"""The host side of a wide main field (hidden_dim = hidden_dim_color = 128) without a GPU: tests/c/wide_pack.cpp is built with g++ from
signerf_amd/csrc/sn_weights.h, sn_layout.h and sn_wide.h alone.  It packs seeded wide fields (appearance dims 0 / 32 / 128, both sh_remap
values), emulates the operand reads of sn_wide_kernels.h on the host -- the float every lane reads from the image as A[i][k] of every
layer, row tile and k-step, against seeded activations in the MFMA's B / D register layout -- and compares with a plain W . x + b in double
(1e-6 relative); then it prints what sn_select_main_wide answers for every (grid, nprop, precision, spacing, box, dump, stats).

A second build with -fsanitize=address,undefined prints the same with no report."""
import os
import re
import subprocess

import pytest

from helpers import ROOT

SRC = os.path.join(ROOT, "tests", "c", "wide_pack.cpp")


def _build_and_run(tmp, name, flags):
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    r = _build_and_run(str(tmp_path_factory.mktemp("wide_pack")), "wide_pack", [])
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def test_packed_image_is_what_the_kernel_reads(plain):
    lines = [ln for ln in plain.splitlines() if ln.startswith("pack ")]
    assert len(lines) == 6
    seen = set()
    for ln in lines:
        m = re.match(r"pack app (\d+) sh_remap (\d) image_floats (\d+) max_rel_err (\S+) (OK|FAIL)$", ln)
        assert m, ln
        seen.add((int(m.group(1)), int(m.group(2))))
        assert int(m.group(3)) == 29476                      # SnWideImg::TOTAL: 117 904 bytes
        assert float(m.group(4)) <= 1e-6 and m.group(5) == "OK", ln
    assert seen == {(a, s) for a in (0, 32, 128) for s in (0, 1)}


def test_selector_table(plain):
    rows = [ln for ln in plain.splitlines() if ln.startswith("select ")]
    assert len(rows) == 2 * 3 * 3 * 2 * 2 * 2 * 2
    chosen = set()
    for ln in rows:
        m = re.match(r"select grid (\d) nprop (\d) prec (\d) spacing (\d) box (\d) dump (\d) stats (\d) -> (.*)$", ln)
        assert m, ln
        grid, nprop, prec, spacing, box, dump, stats = (int(m.group(i)) for i in range(1, 8))
        answer = m.group(8)
        if prec == 2 or dump or stats:
            # refused with SN_ERR_INVALID (1) and a text that says "wide field" and what is not built
            assert answer.startswith("refused 1: wide field") and "not built" in answer, ln
            what = "precision 2" if prec == 2 else ("sn_render_rays_debug" if dump else "march_stats")
            assert what in answer, ln
        else:
            # one instantiation per (sampler mode, grid) serves both spacings and both position maps, in exact fp32 whatever was asked
            assert answer == f"sn_wide_field_main_kernel<{int(nprop > 0)}, {grid}> effective_precision 0", ln
            chosen.add(answer.split(" ")[0] + answer.split(" ")[1])
    assert len(chosen) == 4                                   # SN_WIDE_MAIN_VARIANTS: all four are reachable, nothing else is
    assert "widths (64,64) 1 (128,128) 1 (32,32) 0 (128,64) 0 (64,128) 0" in plain
    m = re.search(r"launch 100x100x128 grid (\d+) lds_bytes (\d+) \(bins (\d+)\) / with proposals (\d+); limit (\d+)", plain)
    assert m
    grid, lds, bins, lds_prop, limit = (int(x) for x in m.groups())
    assert grid == 7 * 7 and lds_prop == 29476 * 4 and lds == lds_prop + bins and bins >= 129 * 4
    assert lds <= limit <= 160 * 1024                         # the CU's LDS


def test_sanitized_build_prints_the_same(plain, tmp_path):
    r = _build_and_run(str(tmp_path), "wide_pack_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    assert r.stdout == plain
