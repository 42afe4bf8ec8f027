"""The optimiser step of include/signerf_hip_optim.h as plain torch ops on the CPU, generic in dtype: every tensor, every scalar and every
intermediate lives in ``dtype`` (fp64: the reference; fp32: what a faithful fp32 implementation loses, the yardstick of the gates).  The
hyper-parameters are what the C ABI carries -- fp32 values -- whatever the dtype of the arithmetic."""
import math

import torch


def f32(x):
    """the fp32 value nearest to a Python float, as a Python float: what a C float field holds"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def group(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, weight_decay=0.0, max_norm=None):
    """a hyper-parameter set whose values are fp32-representable, so that torch.optim.Adam, HipAdam and this file solve one problem"""
    return {"lr": f32(lr), "betas": (f32(betas[0]), f32(betas[1])), "eps": f32(eps), "weight_decay": f32(weight_decay),
            "max_norm": None if max_norm is None else f32(max_norm)}


def grad_norms(tensors, groups, dtype):
    """norm_G per group (of the gradients as they are, still scaled): clip_grad_norm_'s norm of the per-tensor norms; None where nothing clips"""
    out = []
    for j, h in enumerate(groups):
        grads = [t["g"].to(dtype) for t in tensors if t["group"] == j and t["g"].numel()]
        clips = h["max_norm"] is not None and h["max_norm"] > 0 and grads
        out.append(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads])) if clips else None)
    return out


def step(tensors, groups, dtype, grad_scale=None, found_inf=None):
    """tensors: dicts with p, g, m, v (CPU tensors of one shape), step (a float) and group (an index into ``groups``).  Returns the new
    (p, m, v, step) per tensor, in ``dtype``, and the per-group norms."""
    S = lambda x: torch.tensor(float(x), dtype=dtype)
    norms = grad_norms(tensors, groups, dtype)
    out = []
    for t in tensors:
        h = groups[t["group"]]
        p, g, m, v = (t[k].to(dtype) for k in ("p", "g", "m", "v"))
        if found_inf is not None and found_inf != 0:
            out.append((p, m, v, float(t["step"])))
            continue
        now = S(t["step"]) + 1
        inv_scale = S(1) if grad_scale is None else S(1) / S(grad_scale)
        clip = S(1)
        if norms[t["group"]] is not None:
            clip = S(h["max_norm"]) / (norms[t["group"]] / (S(1) if grad_scale is None else S(grad_scale)) + S(1e-6))
            clip = torch.where(clip > 1, S(1), clip)            # (a NaN stays)
        beta1, beta2 = S(h["betas"][0]), S(h["betas"][1])
        g = g * (inv_scale * clip)
        if h["weight_decay"] != 0:
            g = g + S(h["weight_decay"]) * p
        m = m + (1 - beta1) * (g - m)
        v = beta2 * v + (1 - beta2) * (g * g)
        bc1, bc2 = 1 - beta1 ** now, 1 - beta2 ** now
        p = p - (S(h["lr"]) / bc1) * (m / (v.sqrt() / bc2.sqrt() + S(h["eps"])))
        out.append((p, m, v, float(now)))
    return out, norms


def ulp32(x: float) -> float:
    """the spacing of fp32 at |x| (of the smallest normal number below it)"""
    x = abs(float(x))
    if not math.isfinite(x) or x < 2.0 ** -126:
        return 2.0 ** -149
    return 2.0 ** (math.floor(math.log2(x)) - 23)


def gate(got, want64, ref32, steps=1):
    """The project's form, per tensor and output: e_hip <= 2 e_ref32 + steps ulp of the tensor's largest output, e = the largest error
    against the fp64 oracle.  ``steps`` compounds the rounding term over a run of several steps (e_ref32 of the same run has compounded
    already).  Returns (e_hip, e_ref32, bound)."""
    e_hip = float((got.double() - want64).abs().max()) if got.numel() else 0.0
    e_ref = float((ref32.double() - want64).abs().max()) if got.numel() else 0.0
    bound = 2.0 * e_ref + steps * ulp32(float(want64.abs().max()) if got.numel() else 0.0)
    return e_hip, e_ref, bound
