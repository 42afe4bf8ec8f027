/*
 * signerf_hip_optim.h -- companion header of signerf_hip.h: the optimiser step.  torch.optim.Adam (amsgrad=False, maximize=False) over a
 * list of parameter tensors, with torch.nn.utils.clip_grad_norm_ per param group and a GradScaler's unscale / skip folded in: each of
 * param, grad, exp_avg, exp_avg_sq is read once and param, exp_avg, exp_avg_sq are written once.  The formulas are restated in DESIGN.md
 * section 4 "Optimiser step".  Exported from the same libsignerf_hip.so and following the conventions of signerf_hip.h (int status,
 * sn_last_error(NULL) text, caller-owned device memory, work enqueued on the caller's stream, no hidden sync); no handle is needed.
 *
 * The two descriptor arrays are HOST memory (gradients are reallocated every step, so there is nothing to cache).  The library hands them
 * to its kernels as kernel arguments, SN_ADAM_MAX_TENSORS tensors per launch and as many launches as that takes: it makes no
 * host-to-device copy and no sync.  Everything the descriptors point to is DEVICE fp32, dense.
 *
 * Semantics, for one tensor of group G (all of it IEEE fp32 without contraction, square root and division correctly rounded; the
 * per-tensor scalars 1 - beta^t, sqrt(1 - beta2^t) and lr / (1 - beta1^t) are formed in fp64 and rounded once, 1 - beta in fp64 from the
 * fp32 beta and rounded once).  `step` is the tensor's own counter, one device float, as torch's fused=True keeps it:
 *   skip   = found_inf && *found_inf != 0      -> param, exp_avg, exp_avg_sq and step keep their bits
 *   t      = step + 1;  step = t
 *   s      = (grad_scale ? 1 / *grad_scale : 1) * clip_G
 *   g      = grad * s;  if (weight_decay != 0) g = g + weight_decay * p
 *   m      = m + (1 - beta1) * (g - m)
 *   v      = beta2 * v + (1 - beta2) * (g * g)
 *   p      = p - (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
 *   clip_G = max_norm > 0 ? min(1, max_norm / (norm_G / *grad_scale + 1e-6)) : 1      (fp64, rounded once; a NaN norm gives a NaN clip_G)
 *   norm_G = the 2-norm of all gradients of group G that were passed (clip_grad_norm_ with error_if_nonfinite=False), summed in fp64
 * Without a found_inf, non-finite gradients propagate exactly as in torch.  A tensor without a gradient is simply not passed: its step
 * does not advance, as in torch.
 *
 * Reproducibility.  No launch uses a float atomic: norm_G is summed from per-chunk fp64 partial sums in a fixed order, so two calls on
 * the same inputs give the same bits in every output.
 *
 * Argument ranges.  n_tensors == 0 is SN_OK without a launch.  A tensor with n == 0 is ignored without looking at its pointers.
 * SN_ERR_INVALID, before anything is enqueued: a NULL array or required pointer, n < 0, a group outside [0, n_groups), a pointer that is not
 * 4-byte aligned, a beta outside [0, 1), eps < 0, a NaN lr / weight_decay / max_norm, an unknown struct_size (every element of an array
 * carries the same one; the array's stride is that size), a workspace that is NULL, not 8-byte aligned or smaller than
 * sn_adam_workspace_bytes says.  Tensors must not overlap each other.
 *
 * Versioning: SN_OPTIM_ABI_VERSION / sn_optim_abi_version() version THIS header's signatures.
 */
#ifndef SIGNERF_HIP_OPTIM_H
#define SIGNERF_HIP_OPTIM_H

#include "signerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_OPTIM_ABI_VERSION 1
#define SN_ADAM_MAX_TENSORS 32 /* tensors of one launch */
int sn_optim_abi_version(void);

typedef struct {
    uint32_t struct_size; /* sizeof(SnAdamTensor) in the caller's header */
    float* param;         /* [n] */
    const float* grad;    /* [n] */
    float* exp_avg;       /* [n] */
    float* exp_avg_sq;    /* [n] */
    float* step;          /* one float */
    int64_t n;
    int32_t group;        /* index into the group array */
} SnAdamTensor;

typedef struct {
    uint32_t struct_size; /* sizeof(SnAdamGroup) in the caller's header */
    float lr, beta1, beta2, eps, weight_decay;
    float max_norm;       /* <= 0: no clipping */
} SnAdamGroup;

/* One record per element of the tensor array, at the head of the workspace, written by the call for every tensor with n > 0 -- a
 * diagnostic: what the update of that tensor used. */
typedef struct {
    uint32_t skip;        /* 1: the step was skipped (found_inf) */
    float grad_multiplier; /* s */
    float step_size;      /* lr / (1 - beta1^t) */
    float sqrt_bc2;       /* sqrt(1 - beta2^t) */
    double grad_norm;     /* norm_G of the raw (still scaled) gradients; 0 for a group that does not clip */
} SnAdamRecord;

/* total_elements = the sum of n over the tensors.  0 for a negative argument. */
size_t sn_adam_workspace_bytes(int32_t n_tensors, int64_t total_elements);

/* grad_scale, found_inf: one DEVICE float each, either may be NULL.  The workspace must be 8-byte aligned. */
int sn_adam_step(const SnAdamTensor* tensors, int32_t n_tensors, const SnAdamGroup* groups, int32_t n_groups, const float* grad_scale,
                 const float* found_inf, void* workspace, size_t workspace_bytes, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_OPTIM_H */
