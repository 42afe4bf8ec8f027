/*
 * signerf_hip_train_normals.h -- companion header of signerf_hip.h: the analytic normals of TRAINING samples.  nerfstudio's
 * Field.get_normals (restated in oracle.nerfacto.field_analytic_normals) on the parameters the CALLER owns: the hash table of
 * signerf_hip_hashgrid.h and the nn.Linear stack of signerf_hip_mlp.h, as they are while an optimiser rewrites them.  One kernel per call:
 * the hash encoding, the stack forwards, the gradient of its output channel 0 backwards and the contraction with the blend's slopes, with
 * nothing written between them.  The formulas are restated in DESIGN.md section 4 "Training-mode normals".  Exported from the same
 * libsignerf_hip.so and following the conventions of signerf_hip.h (int status, sn_last_error(NULL) text, caller-owned device memory, work
 * enqueued on the caller's stream, no hidden sync); no handle.  sn_render_normals of signerf_hip.h (the handle's uploaded weights, eval
 * only, composited per ray) is a different entry point and is not touched by this one.
 *
 * Arguments.  q [N,3], table [L*T,F], scalings [L], N, L, log2_T, F: as signerf_hip_hashgrid.h has them, with its ranges, its alignment
 * of table and its "Domain".  base_mlp: an SnMlpDesc as sn_mlp_forward takes it (weights [out, in] row-major where torch keeps them; the
 * gradient pointers are ignored) with dims[0] == L * F; anything else is SN_ERR_INVALID.  All tensors are dense fp32 DEVICE memory.
 *
 * Per point: the 8 L corner rows are gathered once -- indexing, corner order and blend nesting exactly those of sn_hashgrid_forward, so
 * the features are that entry point's, bit for bit -- and give the L F features and their three slopes d enc / d o_a, the literal
 * derivative of the blend (signerf_hip_hashgrid.h, grad_q).  The stack runs forwards in sn_mlp_forward's arithmetic; the one-hot gradient
 * of output channel 0 runs backwards through the ReLU masks (torch's: the gradient passes where the activation is not <= 0) and gives
 * g_enc [L F];
 *   g_a = sum_l scalings[l] sum_f g_enc[l,f] slope[l,f,a],     normals = -g / max(|g|, 1e-12)
 * -- F.normalize's rule: a zero gradient gives a zero normal, never a NaN.  fp32 throughout (the exact-fp32 matrix instruction, fmaf
 * chains).  An out-of-domain point gives NaN in all three components of both outputs.  Nothing is shared between points and there are no
 * atomics: two calls on the same inputs give the same bits.
 *
 * The result is a CONSTANT for autograd, as in nerfstudio, whose get_normals calls torch.autograd.grad without create_graph: there is no
 * backward entry point.
 *
 * N >= 0; N == 0 returns SN_OK without a launch and without looking at the data pointers.  What signerf_hip_hashgrid.h and
 * signerf_hip_mlp.h refuse is refused here the same way, before the device is touched and before anything is written.
 *
 * Versioning: SN_TRAIN_NORMALS_ABI_VERSION / sn_train_normals_abi_version() version THIS header's signatures.
 */
#ifndef SIGNERF_HIP_TRAIN_NORMALS_H
#define SIGNERF_HIP_TRAIN_NORMALS_H

#include "signerf_hip.h"
#include "signerf_hip_hashgrid.h"
#include "signerf_hip_mlp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_TRAIN_NORMALS_ABI_VERSION 1
int sn_train_normals_abi_version(void);

/* normals [N,3]: required.  grad_q [N,3], the raw gradient g of the pre-activation density in q: may be NULL. */
int sn_train_normals_analytic(const float* q, const float* table, const float* scalings, int64_t N, int32_t L, int32_t log2_T, int32_t F,
                              const SnMlpDesc* base_mlp, float* normals, float* grad_q, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_TRAIN_NORMALS_H */
