"""The per-sample reference of the normals kernel (tests/normals_oracle.py), on the CPU: the restatement against the oracle's autograd
(fp32) and against finite differences (fp64), the sample set's designed rows, the share of samples a tie excludes, and the gate itself
fed with MUTATED restatements -- a 1 % slope error of any level, a negated d / dz, the dropped zero-offset rule, two exchanged corners and
an ignored ReLU mask must all exceed the limit that tests/test_gpu_normals_samples.py holds the kernel to (the same gate, the same factor).  No GPU."""
import pytest
import torch

import normals_oracle as no
from helpers import onf
from oracle import tcnn_layout as tl

D = torch.float64
# Restatement in fp32 against torch autograd in fp32, per component of the unit normal.  Measured over every case of all_cases(): max 2.6e-6
# (torch grid; 3.9e-6 tiny-cuda-nn), median 6e-8, no sample beyond 1e-4 -- the two differ in the order of the sums only.  Limit = 4 x that
# maximum.
RESTATEMENT_LIMIT = 1.6e-5


def _unit(img):
    """The rendered [0, 1] form back to the unit vector."""
    return img * 2 - 1


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", no.all_cases(), ids=no.case_id)
def test_restatement_in_fp32_agrees_with_the_oracles_autograd(c):
    _, params, ocfg, rays, ref = no.case(*c)
    a32 = no.analytic(params, ocfg, ref["q"], torch.float32)
    want_n = onf.field_analytic_normals(params, ocfg, ref["pos"][:, None])[:, 0]
    want_p = onf.field_pred_normals(params, ocfg, ref["pos"][:, None], a32["h"][:, None])[:, 0]
    dn = (a32["n"] - want_n).abs().max(-1).values
    dp = (no.predicted(params, ocfg, ref["pos"], a32["h"], torch.float32) - want_p).abs().max(-1).values
    print(f"{no.case_id(c)}: analytic max {float(dn.max()):.2e} median {float(dn.median()):.1e}, beyond 1e-4: {int((dn > 1e-4).sum())}; predicted max {float(dp.max()):.2e}")
    assert float(dn.max()) <= RESTATEMENT_LIMIT and float(dp.max()) <= RESTATEMENT_LIMIT
    # ... and what the oracle renders of them is what get_outputs returned (one sample per ray: the weight cancels)
    assert float((no.rendered(want_n, ref["weights"]).float() - ref["ref32"]["normals"]).abs().max()) <= 2.0**-23
    assert bool(torch.isfinite(ref["ref32"]["normals"]).all() and torch.isfinite(ref["ref64"]["normals"]).all())
    # unit vectors -- but for a lattice vertex of every live level (offset 0 on all three axes: no slope left, the normal is 0, rendered 0.5)
    norm = _unit(ref["ref64"]["normals"]).norm(dim=-1)
    assert bool((((norm - 1).abs() <= 1e-8) | ((norm <= 1e-9) & ref["exact_face"] & rays["lattice"])).all())


def test_position_encodings_are_the_oracles():
    x = torch.cat([torch.randn(500, 3, generator=torch.Generator().manual_seed(1)) * 3, torch.tensor([[1e2, -1e4, 1e6], [0.0, 0.25, -0.5]])])
    assert torch.equal(no.frequency_encoding(x, "torch"), onf.nerf_encoding(x))
    assert torch.equal(no.frequency_encoding(x.double(), "torch"), onf.nerf_encoding(x.double()))
    assert torch.equal(no.frequency_encoding(x, "tcnn"), tl.frequency_encoding(x, 2))
    assert float((no.frequency_encoding(x.double(), "tcnn").float() - tl.frequency_encoding(x, 2)).abs().max()) == 0.0


@pytest.mark.parametrize("c", [("torch", None, 1.0, "contract", "piecewise"), ("torch", (3, 4), 1.0, "contract", "piecewise"), ("torch", (15,), 1.0, "box", "piecewise"),
                               ("tcnn", None, 1.0, "contract", "piecewise"), ("tcnn", (1, 2), 1.0, "contract", "piecewise")], ids=no.case_id)
def test_restatement_equals_central_differences_in_fp64(c):
    """d h0 / d q by hand against (h0(q + h e_a) - h0(q - h e_a)) / 2h in fp64, cells and all evaluated at the moved q.  Interior samples only:
    every in-voxel offset of every live level in [0.01, 0.99] and h = 1e-3 / s_max, so that q +- h stays in its voxel at the finest live level
    (where the blend is linear along an axis: the central difference has no truncation error), and the same ReLU mask at all seven points.
    Both sides take their cells from the fp64 q here (the reference proper takes them from fp32 q: its offsets differ by ~1e-7 x)."""
    _, params, ocfg, _, ref = no.case(*c)
    grid = no.grid_of(params, ocfg)
    live = no.live_levels(grid)
    q = ref["q"]
    off = no.cells(q, grid)[1][:, live]
    inner = ((off >= 0.01) & (off <= 0.99)).flatten(1).all(1) & ref["keep"]
    q64 = q[inner].double()
    h = 1e-3 / float(grid["scales"][live].max())
    _, mask0 = no.h0_at(params, ocfg, q64)
    same = torch.ones(q64.shape[0], dtype=torch.bool)
    fd = torch.zeros_like(q64)
    for a in range(3):
        e = torch.zeros(3, dtype=D)
        e[a] = h
        hp, mp = no.h0_at(params, ocfg, q64 + e)
        hm, mm = no.h0_at(params, ocfg, q64 - e)
        fd[:, a] = (hp - hm) / (2 * h)
        same &= (mp == mask0).all(1) & (mm == mask0).all(1)
    g = no.analytic(params, ocfg, q64)["g_q"]
    err = (fd - g)[same].abs().max(-1).values / g[same].abs().max(-1).values
    print(f"{no.case_id(c)}: {int(same.sum())} interior samples of {q.shape[0]}, step {h:.1e}, worst |fd - g| / |g| {float(err.max()):.1e}")
    assert int(same.sum()) >= 300
    # rounding of the difference quotient alone: ~ 2^-50 |h0| / h = 1e-12 s_max |h0| against |g| ~ 1e-2 .. 1 s_max |h0|
    assert float(err.max()) <= 1e-8


# ---- the sample sets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contract", "box"])
def test_sample_set_holds_its_designed_rows(kind):
    c = ("torch", None, 1.0, kind, "piecewise")
    _, params, ocfg, rays, ref = no.case(*c)
    q = ref["q"]
    assert q.shape == (no.N_RAYS, 3) and no.FRAME[0] * no.FRAME[1] == no.N_RAYS and no.N_RAYS % 64 == 5
    assert bool(ref["selector"].all()) and float(q.min()) > 0 and float(q.max()) < 1
    x0 = q[rays["lattice"]] * 16.0                                                  # level 0
    zeros = (x0 == torch.floor(x0)).sum(1)
    assert [int((zeros == k).sum()) for k in (1, 2, 3)] == [no.N_LATTICE // 3] * 3    # offsets of exactly 0 on 1, 2 and 3 axes
    if kind == "contract":
        far = q[rays["far_rows"]]
        assert int(rays["far_rows"].sum()) == no.N_FAR and float(torch.minimum(far, 1 - far).min(1).values.max()) <= 5e-3
        assert float(q.min()) <= 1e-6 and float(q.max()) >= 1 - 1e-6                  # the first and the last cell of every level
        pos = ref["pos"]
        assert int((pos.abs().max(1).values >= 1).sum()) >= 1000                      # the contraction branch
    assert int((ref["exact_face"] & ~rays["lattice"]).sum()) >= (3 if kind == "contract" else 1)    # random rows exactly on a face of some level
    assert float(ref["weights"].min()) >= no.MIN_WEIGHT


@pytest.mark.parametrize("c", no.all_cases(), ids=no.case_id)
def test_ties_exclude_at_most_two_percent(c):
    _, _, _, _, ref = no.case(*c)
    n = ref["keep"].numel()
    print(f"{no.case_id(c)}: {int(ref['relu_tie'].sum())} ReLU ties, {int(ref['near_face'].sum())} near a face, {int(ref['exact_face'].sum())} exactly on one, of {n}")
    assert int((~ref["keep"]).sum()) <= no.MAX_EXCLUDED * n
    assert float(ref["weights"][ref["keep"]].min()) >= no.MIN_WEIGHT


# ---- the gate can fail -------------------------------------------------------------------------------------------------------------------
def _mutant_gate(c, mutant, rows=None):
    _, params, ocfg, _, ref = no.case(*c)
    got = no.rendered(no.analytic(params, ocfg, ref["q"], mutant=mutant)["n"], ref["weights"])
    rows = ref["keep"] if rows is None else rows & ref["keep"]
    ok, e, e_ref, limit = no.gate(got, ref["ref64"]["normals"], ref["ref32"]["normals"], rows)
    clean = no.gate(ref["ref64"]["normals"], ref["ref64"]["normals"], ref["ref32"]["normals"], rows)
    assert clean[0] and clean[1] == 0.0
    return ok, e, limit, int(rows.sum())


def _torch(levels):
    return ("torch", levels, 1.0, "contract", "piecewise")


@pytest.mark.parametrize("level", range(16))
@pytest.mark.parametrize("factor", [1.01, 0.99])
def test_mutant_one_percent_slope_error_of_any_level(level, factor):
    """A uniform factor on the only live level normalises away: the pair cases see it (its neighbour keeps the right scale)."""
    for pair in [p for p in no.PAIRS if level in p]:
        ok, e, limit, _ = _mutant_gate(_torch(pair), no.Mutant(slope_level=level, slope_factor=factor))
        print(f"level {level} x {factor} in L{pair[0]}+{pair[1]}: error {e:.2e}, limit {limit:.2e}")
        assert not ok and e > 100 * limit
    ok, e, limit, _ = _mutant_gate(_torch(None), no.Mutant(slope_level=level, slope_factor=factor))
    print(f"level {level} x {factor} among all levels: error {e:.2e}, limit {limit:.2e}")
    assert not ok


@pytest.mark.parametrize("level", [0, 7, 9, 11, 15])
@pytest.mark.parametrize("feature", [0, 1])
def test_mutant_negated_dz_of_one_feature(level, feature):
    ok, e, limit, _ = _mutant_gate(_torch((level,)), no.Mutant(negate_dz=(level, feature)))
    print(f"d / dz of feature {feature} of level {level} negated: error {e:.2e}, limit {limit:.2e}")
    assert not ok and e > 100 * limit


@pytest.mark.parametrize("levels", [(0,), (5,), (0, 1), None])
def test_mutant_dropped_zero_offset_rule(levels):
    """Judged on the samples exactly on a face: everywhere else floor + 1 IS the ceil corner and the mutant is the restatement."""
    c = _torch(levels)
    ref = no.case(*c)[4]
    ok, e, limit, n = _mutant_gate(c, no.Mutant(keep_zero_offset=True), rows=ref["exact_face"])
    print(f"zero-offset rule dropped, {n} samples exactly on a face: error {e:.2e}, limit {limit:.2e}")
    assert n >= 60 and not ok and e > 100 * limit
    ok, e, _, _ = _mutant_gate(c, no.Mutant(keep_zero_offset=True), rows=~ref["exact_face"])
    assert ok and e == 0.0


@pytest.mark.parametrize("level", [0, 8, 10, 12])
def test_mutant_exchanged_corners(level):
    ok, e, limit, _ = _mutant_gate(_torch((level,)), no.Mutant(swap_corners_level=level))
    print(f"corners 1 <-> 3 of level {level}: error {e:.2e}, limit {limit:.2e}")
    assert not ok and e > 100 * limit


@pytest.mark.parametrize("c", [_torch(None), _torch((4,)), ("tcnn", None, 1.0, "contract", "piecewise")], ids=no.case_id)
def test_mutant_ignored_relu_mask(c):
    _, params, ocfg, _, ref = no.case(*c)
    z1 = no.analytic(params, ocfg, ref["q"])["z1"]
    unit = int(((z1 <= 0) & ref["keep"][:, None]).sum(0).argmax())
    assert int((z1[:, unit] <= 0).sum()) >= 100
    ok, e, limit, _ = _mutant_gate(c, no.Mutant(ignore_relu_unit=unit))
    print(f"ReLU mask of unit {unit} ignored: error {e:.2e}, limit {limit:.2e}")
    assert not ok and e > 100 * limit
