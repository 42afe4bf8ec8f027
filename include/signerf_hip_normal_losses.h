/*
 * signerf_hip_normal_losses.h -- companion header of signerf_hip.h: the per-ray normal terms of a training step, an extension of the
 * "Training back half" family of signerf_hip_losses.h in a header of its own (that header's ABI version stands).  nerfstudio's
 * orientation_loss and pred_normal_loss (model_components/losses.py) and the NormalsRenderer + NormalsShader pair
 * (oracle.nerfacto.render_normals), in one pass over the samples, and the one gradient nerfacto's call needs.  The formulas are restated
 * in DESIGN.md section 4 "Training-mode normals".  Same conventions as signerf_hip_losses.h: all tensors are DEVICE fp32, row-major and
 * dense; R >= 0 rays, 1 <= S <= SN_LOSSES_MAX_SAMPLES samples per ray; R == 0 returns SN_OK without a launch and without looking at the
 * pointers; a negative R, an S outside its range and a NULL required pointer are SN_ERR_INVALID.  One wave works on one ray, the sums
 * over a ray's samples are fp64 and rounded to fp32 once; there are no atomics, so two calls on the same inputs give the same bits.  A
 * non-finite input affects its own ray only.
 *
 * Versioning: SN_NORMAL_LOSSES_ABI_VERSION / sn_normal_losses_abi_version() version THIS header's signatures.
 */
#ifndef SIGNERF_HIP_NORMAL_LOSSES_H
#define SIGNERF_HIP_NORMAL_LOSSES_H

#include "signerf_hip.h"
#include "signerf_hip_losses.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_NORMAL_LOSSES_ABI_VERSION 1
int sn_normal_losses_abi_version(void);

/* weights [R,S], normals [R,S,3]: required.  pred_normals [R,S,3]: required by pred_normal and rendered_pred_normals.
 * directions [R,3] (the rays' directions; the view direction is their negative): required by orientation.
 *   orientation [R]           = sum_s w fmin(0, n . (-d))^2      torch.fmin: a NaN dot product contributes w * 0
 *   pred_normal [R]           = sum_s w (1 - n . n_pred)
 *   rendered_normals [R,3]    = (v / (|v| + 1e-10) + 1) / 2,  v = sum_s w n
 *   rendered_pred_normals [R,3]: the same of n_pred
 * Each output may be NULL, not all four. */
int sn_loss_normals_forward(const float* weights, const float* normals, const float* pred_normals, const float* directions, int64_t R,
                            int32_t S, float* orientation, float* pred_normal, float* rendered_normals, float* rendered_pred_normals,
                            SnStream stream);

/* grad_pred_normals [R,S,3] = grad_pred_normal_r w (-n).  The weights and the analytic normals are detached in nerfacto's call, and the
 * orientation term reads constants only: nothing else gets a gradient. */
int sn_loss_normals_backward(const float* weights, const float* normals, const float* grad_pred_normal, int64_t R, int32_t S,
                             float* grad_pred_normals, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_NORMAL_LOSSES_H */
