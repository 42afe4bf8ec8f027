/*
 * signerf_hip_losses.h -- companion header of signerf_hip.h: the back half of a training step.  What nerfacto / SIGNeRF do AFTER the field
 * has produced per-sample densities and colours: differentiable compositing (RaySamples.get_weights and the training-mode RGB and
 * accumulation renderers) and the two sampler losses (lossfun_distortion, lossfun_outer of nerfstudio's model_components/losses.py), each
 * with a forward and a backward entry point.  The formulas are restated in DESIGN.md section 4 "Training back half".  Exported from the
 * same libsignerf_hip.so and following the conventions of signerf_hip.h (int status, sn_last_error(NULL) text, caller-owned device memory,
 * work enqueued on the caller's stream, no hidden sync); no handle is needed.
 *
 * Common to every entry point: all tensors are DEVICE fp32, row-major and dense.  R >= 0 rays, 1 <= S <= SN_LOSSES_MAX_SAMPLES samples per
 * ray (and 1 <= P <= SN_LOSSES_MAX_SAMPLES envelope intervals).  R == 0 returns SN_OK without a launch (and without
 * looking at the pointers: an empty tensor's may be NULL); a negative R, an S or P outside
 * its range and a NULL required pointer are SN_ERR_INVALID.  One wave works on one ray; per-ray running sums are fp64; there are no
 * atomics, so two calls on the same inputs give the same bits.  A non-finite input affects its own ray only.
 *
 * Versioning: SN_LOSSES_ABI_VERSION / sn_losses_abi_version() version THIS header's signatures.
 */
#ifndef SIGNERF_HIP_LOSSES_H
#define SIGNERF_HIP_LOSSES_H

#include "signerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_LOSSES_ABI_VERSION 1
#define SN_LOSSES_MAX_SAMPLES 1024
int sn_losses_abi_version(void);

/* Compositing, training semantics (no clamp, no nan_to_num on the colours: those are the eval renderer's):
 *   dd = deltas * density, alpha = 1 - exp(-dd), T_i = exp(-sum_{j<i} dd_j), w = nan_to_num(alpha T), acc = sum w,
 *   rgb = sum w_i c_i + bg (1 - acc).
 *   deltas, density [R,S]: required.  colour [R,S,3]: required when rgb is asked for, else may be NULL.
 *   background  DEVICE [3], a constant colour, or NULL: "last_sample", bg = c_{S-1}.
 *   weights [R,S], rgb [R,3], accumulation [R]: outputs, each may be NULL, not all three. */
int sn_loss_composite_forward(const float* deltas, const float* density, const float* colour, const float* background, int64_t R, int32_t S,
                              float* weights, float* rgb, float* accumulation, SnStream stream);

/* Backward of the above: one reverse scan per ray.
 *   grad_weights [R,S], grad_rgb [R,3], grad_acc [R]: the incoming gradients; a NULL one counts as zeros (grad_weights is NULL when only
 *   rgb and accumulation were used).  grad_rgb needs colour.
 *   grad_density [R,S]: required.  grad_colour [R,S,3]: may be NULL; needs colour.  With the "last_sample" background the dependence of
 *   bg on c_{S-1} is part of grad_colour.  A constant background gets no gradient.
 * deltas get NO gradient: nerfacto's samplers hand out detached bins, so nothing upstream could use it. */
int sn_loss_composite_backward(const float* deltas, const float* density, const float* colour, const float* background, int64_t R, int32_t S,
                               const float* grad_weights, const float* grad_rgb, const float* grad_acc, float* grad_density,
                               float* grad_colour, SnStream stream);

/* lossfun_distortion(t [R,S+1], w [R,S]) -> loss [R]:  u_i = (t_i + t_{i+1}) / 2,
 *   loss = sum_i sum_j w_i w_j |u_i - u_j| + (1/3) sum_i w_i^2 (t_{i+1} - t_i)      (the pairwise form, S^2 fp64 multiply-adds per ray) */
int sn_loss_distortion_forward(const float* t, const float* w, int64_t R, int32_t S, float* loss, SnStream stream);

/* grad_w [R,S] = grad_loss_r (2 sum_j w_j |u_i - u_j| + (2/3) w_i (t_{i+1} - t_i)); t is a constant. */
int sn_loss_distortion_backward(const float* t, const float* w, const float* grad_loss, int64_t R, int32_t S, float* grad_w, SnStream stream);

/* lossfun_outer(t [R,S+1], w [R,S], t_env [R,P+1], w_env [R,P]) -> loss [R], the per-ray MEAN over the S samples of
 *   max(w_i - w_outer_i, 0)^2 / (w_i + 1e-7),  w_outer_i = sum_{j = lo_i .. hi_i} w_env_j,
 *   lo_i = clamp(searchsorted(t_env[:-1], t_i, right) - 1, 0, P-1),  hi_i = clamp(searchsorted(t_env[1:], t_{i+1}, right), 0, P-1).
 * t and t_env must be non-decreasing along a ray (they are bin edges).
 *   loss [R] and w_outer [R,S] (nerfstudio's `outer`, for inspection and tests): outputs, either may be NULL, not both; w may be NULL when
 *   loss is. */
int sn_loss_interlevel_forward(const float* t, const float* w, const float* t_env, const float* w_env, int64_t R, int32_t S, int32_t P,
                               float* loss, float* w_outer, SnStream stream);

/* grad_w_env [R,P]_j = sum_{i: lo_i <= j <= hi_i} -2 max(w_i - w_outer_i, 0) / (w_i + 1e-7) grad_loss_r / S.  Only the envelope's weights
 * get a gradient: t, w and t_env are detached in nerfacto's interlevel loss. */
int sn_loss_interlevel_backward(const float* t, const float* w, const float* t_env, const float* w_env, const float* grad_loss, int64_t R,
                                int32_t S, int32_t P, float* grad_w_env, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_LOSSES_H */
