"""The fused Adam step on the GPU (include/signerf_hip_optim.h, signerf_amd/optimizers.py) against tests/optim_oracle.py: one step from a
given state over tensor sets that reach every path of the kernels, weight decay and clipping, a GradScaler's scale and skip, non-finite
gradients, a 100-step trajectory, and optimiser state moving between torch.optim.Adam and HipAdam.

The gate, per tensor and output (p, m, v): e_hip <= 2 e_ref32 + 1 ulp of the tensor's largest output, e = the largest error against the fp64
oracle, ref32 = the same oracle in fp32; ``step`` is exact.  Gradients are exactly 0 or of magnitude 1e-8 .. 1e4, so g g is a normal fp32
number (the subnormal case is written down in DESIGN.md §4 "Optimiser step", not gated)."""
import pytest
import torch

import optim_oracle as oo
from signerf_amd.optimizers import HipAdam, records_of

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 65539]
G0 = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15)
G1 = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-15)


def _tensor_set(sizes, seed, unaligned=(), without_grad=(), steps=(0.0, 1.0, 999.0), one_element_group=False):
    """CPU fp32 dicts p, g, m, v, step, group, and how each goes to the device: ``unaligned`` tensors start one element into their storage."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(sizes):
        mag = 10.0 ** (torch.rand(n, generator=gen) * 12.0 - 8.0)
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        g = torch.where(torch.rand(n, generator=gen) < 0.1, torch.zeros(n), mag * sign)
        t = {"p": torch.randn(n, generator=gen), "g": g, "m": 0.1 * torch.randn(n, generator=gen), "v": 0.01 * torch.rand(n, generator=gen),
             "step": steps[i % len(steps)], "group": i % 2, "unaligned": i in unaligned, "has_grad": i not in without_grad}
        if one_element_group:
            t["group"] = 1 if (n == 1 and not any(o["group"] == 1 for o in out)) else 0
        out.append(t)
    return out


def _to_device(t, key, gpu):
    if not t["unaligned"]:
        return t[key].to(gpu)
    store = torch.zeros(t[key].numel() + 1, device=gpu)
    store[1:] = t[key].to(gpu)
    view = store[1:]
    assert view.data_ptr() % 16 == 4 or view.numel() == 0
    return view


def _hip_optimizer(tensors, groups, gpu):
    """A HipAdam with one param group per hyper-parameter set, its state and gradients put in place."""
    params = [torch.nn.Parameter(_to_device(t, "p", gpu)) for t in tensors]
    opt = HipAdam([{"params": [p for p, t in zip(params, tensors) if t["group"] == j], **h} for j, h in enumerate(groups)])
    for p, t in zip(params, tensors):
        assert p.data_ptr() % 16 == (4 if t["unaligned"] and p.numel() else 0) or p.numel() == 0
        if p.numel():
            opt.state[p] = {"step": torch.tensor(t["step"], device=gpu), "exp_avg": _to_device(t, "m", gpu), "exp_avg_sq": _to_device(t, "v", gpu)}
        if t["has_grad"]:
            p.grad = _to_device(t, "g", gpu)
    return opt, params


def _check_step(tensors, groups, gpu, label, table, grad_scale=None):
    opt, params = _hip_optimizer(tensors, groups, gpu)
    opt.step()
    torch.cuda.synchronize()
    live = [t for t in tensors if t["has_grad"] and t["p"].numel()]
    want, norms = oo.step(live, groups, torch.float64, grad_scale)
    ref, _ = oo.step(live, groups, torch.float32, grad_scale)
    it = iter(zip(want, ref))
    for p, t in zip(params, tensors):
        st = opt.state.get(p, {})
        if not (t["has_grad"] and t["p"].numel()):      # no gradient, or no element: nothing moves, the step does not advance
            assert torch.equal(p.detach().cpu(), t["p"])
            if st:
                assert float(st["step"]) == t["step"] and torch.equal(st["exp_avg"].cpu(), t["m"]) and torch.equal(st["exp_avg_sq"].cpu(), t["v"])
            continue
        (p64, m64, v64, now), (p32, m32, v32, _) = next(it)
        assert float(st["step"]) == now == t["step"] + 1
        for name, got, w64, r32 in (("p", p.detach(), p64, p32), ("m", st["exp_avg"], m64, m32), ("v", st["exp_avg_sq"], v64, v32)):
            e_hip, e_ref, bound = oo.gate(got.cpu(), w64, r32)
            key = (label, name)
            table[key] = max(table.get(key, (0.0, 0.0)), (e_hip / max(bound, 1e-300), e_hip))
            assert e_hip <= bound, (label, name, t["p"].numel(), t["unaligned"], t["step"], e_hip, e_ref, bound)
    return opt, params, live, norms


def _print(table):
    for (label, name), (ratio, e) in sorted(table.items()):
        print(f"[optim] {label:34s} {name}: largest e_hip {e:.3e}, {ratio:.3f} of its bound")


# ---- one step from a given state -----------------------------------------------------------------------------------------------------------
def test_one_step_from_a_given_state(gpu):
    """Every size of SIZES, nonzero m and v, step 0 / 1 / 999, two groups with different hyper-parameters, eps = 1e-15; one view that starts
    one element into its storage (the scalar path), a tensor of size 65539 on each path, a zero-sized tensor, a tensor without a gradient;
    and a set of 70 tensors (one launch takes 32)."""
    groups = [oo.group(**G0), oo.group(**G1)]
    table = {}
    a = _tensor_set(SIZES + [0, 257, 65539, 1023], seed=1, unaligned={5, 11}, without_grad={10})
    _check_step(a, groups, gpu, "every size, 13 tensors", table)
    b = _tensor_set([SIZES[i % 8] for i in range(69)] + [65539], seed=2, unaligned={3, 40, 69})
    opt, params, live, _ = _check_step(b, groups, gpu, "70 tensors, three launches", table)
    recs = records_of(opt._workspace, len(live))
    assert all(r["skip"] == 0 and r["grad_multiplier"] == 1.0 and r["grad_norm"] == 0.0 for r in recs)
    _print(table)


# ---- weight decay and clipping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norms", [(1e-2, 1e7), (1e7, 1.0)], ids=["clip-group-0", "clip-group-1"])
def test_weight_decay_and_max_norm(gpu, max_norms):
    """Each group once with its norm above max_norm (it clips) and once below (clip_G = 1); weight decay in both.  norm_G is the fp64 norm at
    2^-24 relative, and a second call on the same inputs gives the same bits in every output."""
    groups = [oo.group(weight_decay=0.01, max_norm=max_norms[0], **G0), oo.group(weight_decay=0.1, max_norm=max_norms[1], **G1)]
    table = {}
    tensors = _tensor_set([SIZES[i % 9] for i in range(40)], seed=3, unaligned={7, 17})
    opt, params, live, norms = _check_step(tensors, groups, gpu, "40 tensors, wd, max_norm", table)
    recs = records_of(opt._workspace, len(live))
    order = [t for j in range(2) for t in live if t["group"] == j]      # HipAdam passes its param groups one after the other
    for r, t in zip(recs, order):
        want = float(norms[t["group"]])
        assert abs(r["grad_norm"] - want) <= 2.0 ** -24 * want, (r, want)
        clip = min(1.0, groups[t["group"]]["max_norm"] / (want + 1e-6))
        assert r["grad_multiplier"] == pytest.approx(clip, rel=2.0 ** -23) and (clip < 1.0) == (groups[t["group"]]["max_norm"] < 1e3)
    again, params2 = _hip_optimizer(tensors, groups, gpu)
    again.step()
    for p, q in zip(params, params2):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k].view(torch.int32), again.state[q][k].view(torch.int32))
    assert records_of(again._workspace, len(live)) == recs
    _print(table)


def test_a_group_of_one_element_clips(gpu):
    groups = [oo.group(max_norm=0.5, **G0), oo.group(max_norm=0.5, weight_decay=0.01, **G1)]
    table = {}
    tensors = _tensor_set([257, 1, 5], seed=4, one_element_group=True)
    tensors[1]["g"] = torch.tensor([-3.0])
    assert [t["group"] for t in tensors] == [0, 1, 0]
    opt, params, live, norms = _check_step(tensors, groups, gpu, "a group of one element", table)
    recs = records_of(opt._workspace, 3)
    assert float(norms[1]) == 3.0 and recs[2]["grad_norm"] == 3.0 and recs[2]["grad_multiplier"] == pytest.approx(0.5 / (3.0 + 1e-6), rel=2.0 ** -23)
    _print(table)


# ---- grad scaling ----------------------------------------------------------------------------------------------------------------------------
def _bits(opt, params):
    return [(p.detach().view(torch.int32).clone(), {k: opt.state[p][k].view(torch.int32).clone() for k in ("step", "exp_avg", "exp_avg_sq")})
            for p in params if p.numel() and p in opt.state]


def _same(a, b):
    return all(torch.equal(x[0], y[0]) and all(torch.equal(x[1][k], y[1][k]) for k in x[1]) for x, y in zip(a, b)) and len(a) == len(b)


def test_a_power_of_two_grad_scale_gives_the_unscaled_bits_and_found_inf_keeps_every_bit(gpu):
    groups = [oo.group(max_norm=1.0, weight_decay=0.01, **G0), oo.group(**G1)]
    tensors = _tensor_set([SIZES[i % 9] for i in range(36)], seed=5, unaligned={4})
    plain, pp = _hip_optimizer(tensors, groups, gpu)
    before = _bits(plain, pp)
    plain.step()
    scaled_t = [dict(t, g=t["g"] * 65536.0) for t in tensors]
    scaled, sp = _hip_optimizer(scaled_t, groups, gpu)
    scaled.grad_scale, scaled.found_inf = torch.tensor(65536.0, device=gpu), torch.zeros(1, device=gpu)
    scaled.step()
    assert _same(_bits(plain, pp), _bits(scaled, sp)) and not _same(before, _bits(plain, pp))
    rp, rs = records_of(plain._workspace, 36), records_of(scaled._workspace, 36)
    assert all(a["grad_norm"] * 65536.0 == b["grad_norm"] and a["grad_multiplier"] == b["grad_multiplier"] * 65536.0 for a, b in zip(rp, rs))
    skipped, kp = _hip_optimizer(scaled_t, groups, gpu)
    skipped.grad_scale, skipped.found_inf = torch.tensor(65536.0, device=gpu), torch.ones(1, device=gpu)
    skipped.step()
    assert _same(before, _bits(skipped, kp)) and all(r["skip"] == 1 for r in records_of(skipped._workspace, 36))


def test_a_stock_grad_scaler_skips_an_inf_step_and_a_clean_step_is_the_unscaled_one(gpu):
    gen = torch.Generator().manual_seed(6)
    coef = [torch.randn(n, generator=gen) for n in (257, 5, 1023)]
    start = [torch.randn(n, generator=gen) for n in (257, 5, 1023)]

    def run(scaler, poison):
        params = [torch.nn.Parameter(s.to(gpu)) for s in start]
        opt = HipAdam(params, **oo.group(max_norm=1.0, **G0))
        for k in range(2):
            c = [x.clone() for x in coef]
            if poison and k == 1:
                c[1][2] = float("inf")
            loss = sum((p * x.to(gpu)).sum() for p, x in zip(params, c))
            opt.zero_grad()
            if scaler is None:
                loss.backward()
                opt.step()
            else:
                scaler.scale(loss).backward()
                scaler.step(opt)
                scaler.update()
        return opt, params

    ref, rp = run(None, False)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    got, gp = run(scaler, False)
    assert _same(_bits(ref, rp), _bits(got, gp)) and scaler.get_scale() == 65536.0 and float(got.state[gp[0]]["step"]) == 2.0
    assert not hasattr(got, "grad_scale") and not hasattr(got, "found_inf")
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    bad, bp = run(scaler, True)
    assert scaler.get_scale() == 32768.0 and all(float(bad.state[p]["step"]) == 1.0 for p in bp)
    assert all(torch.isfinite(p).all() for p in bp)
    # what one clean step leaves: the second, poisoned one must have changed nothing
    first = HipAdam([torch.nn.Parameter(s.to(gpu)) for s in start], **oo.group(max_norm=1.0, **G0))
    for p, x in zip(first.param_groups[0]["params"], coef):
        p.grad = x.to(gpu)
    first.step()
    assert _same(_bits(first, first.param_groups[0]["params"]), _bits(bad, bp))


def test_without_a_scaler_a_nan_gradient_poisons_the_elements_torch_poisons(gpu):
    for max_norm in (None, 1.0):
        tensors = _tensor_set([257, 1023, 5], seed=7)
        for t in tensors:
            t["group"] = 0
        tensors[1]["g"][[0, 511, 1022]] = float("nan")
        tensors[0]["g"][100] = float("inf")
        h = oo.group(max_norm=max_norm, **G0)
        opt, params = _hip_optimizer(tensors, [h], gpu)
        opt.step()
        theirs = [torch.nn.Parameter(t["p"].to(gpu)) for t in tensors]
        adam = torch.optim.Adam(theirs, lr=h["lr"], betas=h["betas"], eps=h["eps"], foreach=False)
        for q, t in zip(theirs, tensors):
            adam.state[q] = {"step": torch.tensor(t["step"]), "exp_avg": t["m"].to(gpu), "exp_avg_sq": t["v"].to(gpu)}
            q.grad = t["g"].to(gpu)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(theirs, max_norm)
        adam.step()
        for p, q in zip(params, theirs):
            for mine, torchs in ((p.detach(), q.detach()), (opt.state[p]["exp_avg"], adam.state[q]["exp_avg"]), (opt.state[p]["exp_avg_sq"], adam.state[q]["exp_avg_sq"])):
                assert torch.equal(torch.isnan(mine), torch.isnan(torchs)) and torch.equal(torch.isinf(mine), torch.isinf(torchs))
        poisoned = sum(int(torch.isnan(p).sum()) for p in params)
        assert poisoned == (4 if max_norm is None else 257 + 1023 + 5)       # (inf: m = inf, v = inf, inf / inf = NaN)


# ---- trajectory ------------------------------------------------------------------------------------------------------------------------------
def test_a_hundred_steps_of_a_quadratic(gpu):
    """f(p) = sum a (p - c)^2 / 2 plus a fixed pseudo-random gradient term per step, 1000 elements, 100 steps; every gradient is elementwise
    torch ops (no atomics anywhere).  HipAdam, torch.optim.Adam(foreach=False) in fp32 and the fp64 oracle start alike; HipAdam's final error
    against fp64 is gated at twice torch-fp32's own."""
    gen = torch.Generator().manual_seed(8)
    n, steps = 1000, 100
    a, c, p0 = 0.5 + torch.rand(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    noise = 0.1 * torch.randn(steps, n, generator=gen)
    h = oo.group(**G0)
    grad = lambda p, k, dt: a.to(device=p.device, dtype=dt) * (p - c.to(device=p.device, dtype=dt)) + noise[k].to(device=p.device, dtype=dt)
    hp = torch.nn.Parameter(p0.to(gpu))
    hip = HipAdam([hp], **h)
    tp = torch.nn.Parameter(p0.clone())
    adam = torch.optim.Adam([tp], lr=h["lr"], betas=h["betas"], eps=h["eps"], foreach=False)
    state = {"p": p0.double(), "m": torch.zeros(n, dtype=torch.float64), "v": torch.zeros(n, dtype=torch.float64), "step": 0.0, "group": 0}
    for k in range(steps):
        hp.grad = grad(hp.detach(), k, torch.float32)
        hip.step()
        tp.grad = grad(tp.detach(), k, torch.float32)
        adam.step()
        state["g"] = grad(state["p"], k, torch.float64)
        ((p, m, v, now),), _ = oo.step([state], [h], torch.float64)
        state.update(p=p, m=m, v=v, step=now)
    e_hip = float((hp.detach().cpu().double() - state["p"]).abs().max())
    e_torch = float((tp.detach().double() - state["p"]).abs().max())
    moved = float((state["p"] - p0.double()).abs().max())
    print(f"\n[optim] 100-step quadratic: HipAdam {e_hip:.3e}, torch.optim.Adam fp32 {e_torch:.3e} from the fp64 oracle (parameters moved {moved:.3f})")
    assert float(hip.state[hp]["step"]) == steps and moved > 0.3
    assert e_hip <= 2.0 * e_torch


# ---- state exchange --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["torch", "hip"])
def test_state_moves_between_torch_adam_and_hip_adam(gpu, first):
    """Five steps of one optimiser, its state_dict into the other, five more: against ten steps of the oracle, under the single-step gate
    compounded (2 e_ref32 of the ten fp32 steps + 10 ulp).  The gradients are a fixed pseudo-random sequence."""
    gen = torch.Generator().manual_seed(9)
    sizes = [257, 5, 1023]
    h = oo.group(weight_decay=0.01, **G0)
    start = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[torch.randn(n, generator=gen) * 10.0 ** (k % 3 - 1) for n in sizes] for k in range(10)]
    params = [torch.nn.Parameter(s.to(gpu)) for s in start]
    make = {"torch": lambda: torch.optim.Adam(params, lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"], foreach=False),
            "hip": lambda: HipAdam(params, **h)}
    opt = make[first]()
    for k in range(10):
        if k == 5:
            nxt = make["hip" if first == "torch" else "torch"]()
            nxt.load_state_dict(opt.state_dict())
            opt = nxt
        for p, g in zip(params, grads[k]):
            p.grad = g.to(gpu)
        opt.step()
    states = {dt: [{"p": s.to(dt), "m": torch.zeros_like(s, dtype=dt), "v": torch.zeros_like(s, dtype=dt), "step": 0.0, "group": 0} for s in start]
              for dt in (torch.float64, torch.float32)}
    for k in range(10):
        for dt, ts in states.items():
            for t, g in zip(ts, grads[k]):
                t["g"] = g
            out, _ = oo.step(ts, [h], dt)
            for t, (p, m, v, now) in zip(ts, out):
                t.update(p=p, m=m, v=v, step=now)
    for p, t64, t32 in zip(params, states[torch.float64], states[torch.float32]):
        st = opt.state[p]
        assert float(st["step"]) == 10.0
        for name, got, key in (("p", p.detach(), "p"), ("m", st["exp_avg"], "m"), ("v", st["exp_avg_sq"], "v")):
            e_hip, e_ref, bound = oo.gate(got.cpu(), t64[key], t32[key], steps=10)
            print(f"[optim] {first} first, {name} [{p.numel()}]: e {e_hip:.3e}, e_ref32 {e_ref:.3e}, bound {bound:.3e}")
            assert e_hip <= bound, (first, name, p.numel(), e_hip, e_ref, bound)
