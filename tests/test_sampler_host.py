"""Training-mode proposal sampling, CPU side: the restatement tests/sampler_oracle.py against ``oracle.nerfacto`` bit for bit, the Philox
restatement against Random123's known-answer vectors, the companion C header include/signerf_hip_sampler.h against the binding, the
library's exports and its argument refusals (in a child process: nothing is launched), the monotonicity of the restatement on the inputs
the GPU tests use, and ``ProposalNetworkSampler``'s schedule logic with stub density functions.  No GPU."""
import os

import numpy as np
import pytest
import torch

import sampler_oracle as so
from abi_helpers import c99_probe, refusal_sweep, struct_fields
from helpers import ROOT, onf
from signerf_amd import _lib

HEADER = os.path.join(ROOT, "include", "signerf_hip_sampler.h")
# what tests/test_gpu_sampler.py runs
LEVELS = [(1, 1), (2, 257), (65, 64), (256, 96), (96, 48), (8, 1024), (1024, 8)]
ANNEALS = (0.0, 0.35, 1.0)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", LEVELS)
def test_pdf_restatement_with_the_eval_u_is_the_oracle_bit_for_bit(N, M):
    bins, w = so.previous_level(65, N, seed=N + M)
    got, inds, cdf = so.pdf_bins(bins, w, onf.pdf_u(M), anneal=1.0)
    want, want_inds, want_cdf = onf.pdf_sample(bins, w, M)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(inds, want_inds) and torch.equal(cdf.view(torch.int32), want_cdf.view(torch.int32))


@pytest.mark.parametrize("mode", so.MODES)
def test_initial_restatement_without_jitter_is_the_oracle_bit_for_bit(mode):
    """The un-jittered sampler is the base grid itself: the restatement's Euclidean map on it must be ``oracle.nerfacto.initial_sampler``;
    and the jittered bins stay inside their cells."""
    _, _, nears, fars = so.rays(65, 3)
    for N in (1, 48, 256):
        sb, eb = onf.initial_sampler(nears[:, None], fars[:, None], N, mode)
        got = so.euclid(sb.expand(65, N + 1), nears, fars, mode)
        assert torch.equal(got.view(torch.int32), eb.view(torch.int32))
        # the jittered bins stay inside their cells: lower <= bin <= upper, and rand = 0 / 1 are the cell's ends
        base = torch.linspace(0.0, 1.0, N + 1)
        lo, hi = so.initial_bins(base, torch.zeros(65)), so.initial_bins(base, torch.ones(65))
        mid = so.initial_bins(base, so.uniforms(65, N + 1, False, N))
        assert bool((lo <= mid).all()) and bool((mid <= hi).all()) and float(lo[0, 0]) == 0.0 and float(hi[0, -1]) == 1.0
        assert torch.equal(lo[0, 1:], (base[1:] + base[:-1]) / 2) and torch.equal(hi[0, :-1], (base[1:] + base[:-1]) / 2)


def test_samples_restatement_is_the_oracles_position_map():
    o, d, nears, fars = so.rays(33, 5, far_out=True)
    eb = so.euclid(so.initial_bins(torch.linspace(0.0, 1.0, 49), so.uniforms(33, 49, True, 1)), nears, fars, "uniform")
    deltas, pos, q, sel = so.samples(eb, o, d)
    want = onf.sample_positions(o, d, eb[:, :-1, None], eb[:, 1:, None])
    wq, wsel = onf.normalized_positions(want)
    assert torch.equal(pos, want) and torch.equal(q, wq) and torch.equal(sel, wsel) and 0 < int(sel.sum()) < sel.numel()
    assert torch.equal(deltas, eb[:, 1:] - eb[:, :-1])


@pytest.mark.parametrize("N,M", LEVELS)
def test_restatement_bins_are_non_decreasing_on_the_gpu_test_inputs(N, M):
    """The condition tests/test_gpu_sampler.py asserts for the kernel holds for the fp32 restatement on the same inputs (both jitter modes,
    every anneal) -- at the GPU tests' R = 257 for every level pair and at R = 4096 for nerfacto's own (256 -> 96), (96 -> 48)."""
    for R in (257, 4096) if (N, M) in ((256, 96), (96, 48)) else (257,):
        bins, w = so.previous_level(R, N, seed=N + M)
        for single in (True, False):
            u = so.train_u(so.u_grid(M), so.uniforms(R, M + 1, single, seed=M))
            for a in ANNEALS:
                got, _, _ = so.pdf_bins(bins, w, u, anneal=a)
                assert so.decreasing_pairs(got) == 0, (R, single, a)
                assert bool((got >= bins[:, :1]).all()) and bool((got <= bins[:, -1:]).all())


def test_pow_of_zero_to_zero_is_one():
    w = torch.tensor([[0.0, 0.0, 1.0, 0.25]])
    bins = torch.linspace(0, 1, 5)[None]
    flat, _, _ = so.pdf_bins(bins, torch.ones(1, 4), so.u_grid(8)[None], anneal=1.0)
    got, _, _ = so.pdf_bins(bins, w, so.u_grid(8)[None], anneal=0.0)
    assert torch.equal(got, flat)       # anneal = 0: every weight is 1, the zeros included


# ---- Philox --------------------------------------------------------------------------------------------------------------------------------
KAT = [  # Random123 kat_vectors, philox4x32 with 10 rounds: counter, key, result
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_restatement_reproduces_the_known_answer_vectors(ctr, key, want):
    got = so.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key)
    assert tuple(int(x[0]) for x in got) == want


def test_philox_float_conversion_stays_below_one():
    x = np.array([0, 1, 255, 256, 0x7FFFFFFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32)
    f = so.word_to_float(x)
    assert f.dtype == np.float32 and float(f.min()) == 0.0 and float(f.max()) == 1.0 - 2.0**-24 and f[3] == np.float32(2.0**-24)
    u = so.philox_uniform(257, 97, seed=0x0123456789ABCDEF, offset=(5 << 32) | 9, single_jitter=False)
    assert u.shape == (257, 97) and u.dtype == torch.float32 and 0.0 <= float(u.min()) and float(u.max()) < 1.0
    assert 0.45 < float(u.mean()) < 0.55 and u.unique().numel() > 0.99 * u.numel()
    one = so.philox_uniform(257, 97, seed=0x0123456789ABCDEF, offset=(5 << 32) | 9, single_jitter=True)
    assert one.shape == (257,) and torch.equal(one, u[:, 0])     # j = 0 is the single-jitter counter
    assert not torch.equal(u, so.philox_uniform(257, 97, seed=0x0123456789ABCDEF, offset=(5 << 32) | 10, single_jitter=False))


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
NAMES = ["sn_sampler_abi_version", "sn_sampler_initial", "sn_sampler_pdf"]
KERNELS = ["sn_train_sampler_initial_kernel", "sn_train_sampler_pdf_kernel"]


def test_sampler_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    assert sorted(_lib.header("sampler").functions) == NAMES
    assert struct_fields(HEADER, "SnSamplerRays") == [f[0] for f in _lib.SnSamplerRays._fields_]
    assert struct_fields(HEADER, "SnSamplerPdf") == [f[0] for f in _lib.SnSamplerPdf._fields_]
    lib = _lib.load()
    assert lib.sn_sampler_abi_version() == _lib.header("sampler").version == 1
    blob = open(built_lib, "rb").read()
    for k in KERNELS:
        assert 24 <= len(k) <= 99       # (names behind _Z23...: DESIGN.md §4 "Kernel names")
        assert ("_Z%d%s15SnSamplerParams" % (len(k), k)).encode() in blob


def test_sampler_header_compiles_as_c99(tmp_path):
    import ctypes as C

    got = c99_probe(tmp_path, "signerf_hip_sampler.h", "%d %d %d %d",
                    "SN_SAMPLER_ABI_VERSION, SN_SAMPLER_MAX_SAMPLES, (int)sizeof(SnSamplerRays), (int)sizeof(SnSamplerPdf)")
    assert got == ["1", "1024", str(C.sizeof(_lib.SnSamplerRays)), str(C.sizeof(_lib.SnSamplerPdf))]


_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
P = 0x1000   # never dereferenced: every call below is refused (or n_rays == 0) before the device is touched
def rays(**kw):
    r = _lib.SnSamplerRays()
    vals = dict(n_samples=48, n_rays=4, origins=P, directions=P, near_plane=0.05, far_plane=1000.0, spacing_bins=P)
    vals.update(kw)
    for k, v in vals.items():
        setattr(r, k, v)
    return r
def pdf(**kw):
    r = _lib.SnSamplerPdf()
    vals = dict(n_in=96, spacing_bins=P, weights=P, u_grid=P, anneal=1.0, histogram_padding=0.01)
    vals.update(kw)
    for k, v in vals.items():
        setattr(r, k, v)
    return r
def done(st, name):
    msg = lib.sn_last_error(None)
    return "%d:%s" % (st, "text" if (st == 0 or (msg and name.encode() in msg)) else "notext")
def ini(r, base=P):
    return done(lib.sn_sampler_initial(C.byref(r) if r is not None else None, base, N), "sn_sampler_initial")
def res(r, p):
    return done(lib.sn_sampler_pdf(C.byref(r) if r is not None else None, C.byref(p) if p is not None else None, N), "sn_sampler_pdf")
inf, nan = float("inf"), float("nan")
calls = {"abi": lambda: "%d:text" % lib.sn_sampler_abi_version()}
for tag, f in (("ini", lambda r: ini(r)), ("pdf", lambda r: res(r, pdf()))):
    calls.update({
     tag + "_no_rays": lambda f=f: f(None), tag + "_R_neg": lambda f=f: f(rays(n_rays=-1)), tag + "_R_2p31": lambda f=f: f(rays(n_rays=2**31)),
     tag + "_M_0": lambda f=f: f(rays(n_samples=0)), tag + "_M_1025": lambda f=f: f(rays(n_samples=1025)), tag + "_M_neg": lambda f=f: f(rays(n_samples=-3)),
     tag + "_no_origins": lambda f=f: f(rays(origins=N)), tag + "_no_directions": lambda f=f: f(rays(directions=N)),
     tag + "_spacing_mode_2": lambda f=f: f(rays(spacing_mode=2)), tag + "_size_0": lambda f=f: f(rays(struct_size=0)),
     tag + "_size_small": lambda f=f: f(rays(struct_size=C.sizeof(_lib.SnSamplerRays) - 8)),
     tag + "_size_large": lambda f=f: f(rays(struct_size=C.sizeof(_lib.SnSamplerRays) + 8)),
     tag + "_R_0_bad_M": lambda f=f: f(rays(n_rays=0, n_samples=0)),
     "ok_" + tag + "_R_0": lambda f=f: f(rays(n_rays=0)), "ok_" + tag + "_R_0_null": lambda f=f: f(rays(n_rays=0, origins=N, directions=N, spacing_bins=N)),
     "ok_" + tag + "_R_0_M_1024": lambda f=f: f(rays(n_rays=0, n_samples=1024)),
    })
calls.update({
 "ini_no_base": lambda: ini(rays(), base=N), "ok_ini_R_0_no_base": lambda: ini(rays(n_rays=0), base=N),
 "pdf_no_pdf": lambda: res(rays(), None), "pdf_N_0": lambda: res(rays(), pdf(n_in=0)), "pdf_N_1025": lambda: res(rays(), pdf(n_in=1025)),
 "pdf_no_bins": lambda: res(rays(), pdf(spacing_bins=N)), "pdf_no_weights": lambda: res(rays(), pdf(weights=N)), "pdf_no_u": lambda: res(rays(), pdf(u_grid=N)),
 "pdf_anneal_neg": lambda: res(rays(), pdf(anneal=-0.5)), "pdf_anneal_nan": lambda: res(rays(), pdf(anneal=nan)), "pdf_anneal_inf": lambda: res(rays(), pdf(anneal=inf)),
 "pdf_padding_nan": lambda: res(rays(), pdf(histogram_padding=nan)), "pdf_own_size_0": lambda: res(rays(), pdf(struct_size=0)),
 "pdf_own_size_small": lambda: res(rays(), pdf(struct_size=C.sizeof(_lib.SnSamplerPdf) - 4)), "pdf_R_0_bad_anneal": lambda: res(rays(n_rays=0), pdf(anneal=-1.0)),
 "pdf_R_0_bad_N": lambda: res(rays(n_rays=0), pdf(n_in=0)),
 "ok_pdf_R_0_own_null": lambda: res(rays(n_rays=0), pdf(spacing_bins=N, weights=N, u_grid=N)), "ok_pdf_R_0_anneal_0": lambda: res(rays(n_rays=0), pdf(anneal=0.0)),
})
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_sampler_entry_points_refuse_bad_arguments_before_the_device(built_lib):
    """A count outside its range, a NULL required pointer, a struct_size too small or too large, an anneal that is negative or not finite,
    n_rays < 0: SN_ERR_INVALID with the entry point's name in sn_last_error; n_rays = 0 is SN_OK without a launch.  In a child process -- a
    crash would be a segfault -- and host-only."""
    got = refusal_sweep(_SWEEP)
    want = {k: ("0:text" if k.startswith("ok_") else "1:text") for k in got}
    want["abi"] = "1:text"
    assert len(got) == 1 + 2 * 16 + 18 and got == want


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------
def _bundle(R=8):
    from signerf_amd.cameras import RayBundle

    o, d, nears, fars = so.rays(R)
    return RayBundle(origins=o, directions=d, pixel_area=torch.ones(R, 1), camera_indices=torch.zeros(R, 1, dtype=torch.long),
                     nears=nears[:, None], fars=fars[:, None])


def test_python_surface_refuses_before_the_device():
    from signerf_amd import samplers

    b = _bundle()
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        samplers.sample_initial(b, 16)
    b.origins = b.origins.double()
    with pytest.raises(TypeError, match="fp32"):
        samplers.sample_initial(b, 16)
    with pytest.raises(ValueError, match="1..1024"):
        samplers.sample_initial(_bundle(), 1025)
    with pytest.raises(ValueError, match="anneal"):
        samplers.sample_pdf(_bundle(), None, torch.zeros(8, 4, 1), 16, anneal=-1.0)


def test_anneal_schedule_and_update_rule_with_stub_density_functions():
    """nerfstudio's schedule logic needs no kernel: the anneal values ``set_training_step`` hands over at steps 0 / 100 / 1000, and which
    steps evaluate the proposal densities with a gradient (``steps_since_update > update_sched(step) or step < 10``)."""
    from signerf_amd import samplers
    from signerf_amd.config import NerfactoModelConfig

    cfg = NerfactoModelConfig()
    assert (cfg.use_single_jitter, cfg.proposal_update_every, cfg.proposal_warmup) == (True, 5, 5000)
    assert (cfg.use_proposal_weight_anneal, cfg.proposal_weights_anneal_slope, cfg.proposal_weights_anneal_max_num_iters) == (True, 10.0, 1000)
    assert cfg.training_forward is False
    bias = lambda x, b: b * x / ((b - 1) * x + 1)   # noqa: E731
    assert samplers.anneal_at(0, 10.0, 1000) == 0.0 and samplers.anneal_at(1000, 10.0, 1000) == 1.0 and samplers.anneal_at(5000, 10.0, 1000) == 1.0
    assert samplers.anneal_at(100, 10.0, 1000) == pytest.approx(bias(0.1, 10.0)) == pytest.approx(1.0 / 1.9)
    sched = samplers.update_schedule(cfg.proposal_warmup, cfg.proposal_update_every)
    assert sched(0) == 1.0 and sched(5000) == 5.0 and sched(10**6) == 5.0 and sched(2500) == pytest.approx(2.5)

    calls = []
    s = samplers.ProposalNetworkSampler(num_nerf_samples_per_ray=8, num_proposal_samples_per_ray=(16, 12), num_proposal_network_iterations=2,
                                        update_sched=sched, seed=1)
    assert s.single_jitter is True and s.histogram_padding == 0.01 and s._anneal == 1.0
    s.set_anneal(0.25)
    assert s._anneal == 0.25
    updated = []
    for step in range(0, 40):
        s.step_cb(step)
        updated.append(s.will_update())
        if updated[-1]:
            s.mark_updated()
    # every step below 10; then whenever more than update_sched(step) ~ 1.0 steps have passed since the last update
    assert all(updated[:10]) and updated[10:16] == [False, True, False, True, False, True]
    late = samplers.ProposalNetworkSampler(8, (16, 12), 2, update_sched=lambda step: 5.0, seed=1)
    got = []
    for step in range(100, 125):
        late.step_cb(step)
        got.append(late.will_update())
        if got[-1]:
            late.mark_updated()
    assert [i for i, g in enumerate(got) if g] == [5, 11, 17, 23]          # steps_since_update 6 > 5
    with pytest.raises(ValueError, match="iterations"):
        samplers.ProposalNetworkSampler(8, (16,), 2)
    # a CPU bundle reaches the first launch and is refused there; the density functions are never called
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        s(_bundle(), [lambda p: calls.append(p) for _ in range(2)])
    assert calls == []
