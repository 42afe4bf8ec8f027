/*
 * signerf_hip_mlp.h -- companion header of signerf_hip.h: the trainable MLP.  nerfstudio's torch MLP (restated in
 * oracle.nerfacto.mlp_forward) on the weights the CALLER owns -- the nn.Linear parameters an optimiser rewrites every step -- with a forward
 * and a backward entry point.  With it the nn.Linear stacks of a nerfacto field run as one kernel per pass instead of a GEMM, a bias and a
 * ReLU per layer, and no hidden activation is kept for the backward pass.  The formulas are restated in DESIGN.md section 4 "Trainable
 * MLP".  Exported from the same libsignerf_hip.so and following the conventions of signerf_hip.h (int status, sn_last_error(NULL) text,
 * caller-owned device memory, work enqueued on the caller's stream, no hidden sync); no handle and no packing step.  The render kernels'
 * uploaded weight images (sn_upload_weights / sn_finalize_weights) are not touched by these entry points.
 *
 * The network: h_0 = x [N, dims[0]]; for i = 1..n_layers: z_i = h_{i-1} W_i^T + b_i with W_i = weights[i-1] [dims[i], dims[i-1]] row-major
 * (the nn.Linear's own layout) and b_i = biases[i-1] [dims[i]]; h_i = relu(z_i) for i < n_layers; y = z_n [N, dims[n]].  All tensors are
 * dense fp32 DEVICE memory, aligned to 4 bytes.  1 <= n_layers <= SN_MLP_MAX_LAYERS and 1 <= dims[i] <= SN_MLP_MAX_DIM.
 *
 * Arithmetic, SnMlpDesc.precision = SN_MLP_PRECISION_FP32 (0, what a zeroed descriptor asks for): exact fp32 (the f32 matrix instruction, an fmaf chain; no reduced-precision operand).  A layer's output is a chain from 0
 * over its inputs in the order k = 16 t + 4 h + s (t = 0.., s = 0..3, h = 0..3 innermost) with the bias added LAST.  relu(NaN) is NaN, as in
 * torch; the backward mask is torch's: dZ_i = 0 where h_i <= 0, dH_i elsewhere (a NaN activation passes its gradient).  A non-finite value
 * in one row of x stays in that row of y and dx; it reaches the weight gradients, which sum over the rows.
 *
 * Arithmetic, SnMlpDesc.precision = SN_MLP_PRECISION_FP16 (1): the method's mixed precision -- fp16 operands, fp32 accumulation, fp32 master
 * weights (DESIGN.md section 4 "Mixed-precision MLP").  All pointers stay fp32 device memory and the workspace has the same size.  With r16 =
 * round-to-nearest-even to IEEE fp16 (overflow gives +-inf, subnormal results and subnormal operands are kept, NaN stays NaN):
 * h_0 = r16(x); z_i = sum_k r16(W_i)[o][k] h_{i-1}[k] accumulated in fp32, then + b_i[o] in fp32 (the bias is added last and never rounded);
 * h_i = r16(relu(z_i)); y = z_n in fp32.  Backward: the h_i are recomputed, bit for bit the forward's; dZ_n = r16(grad_y);
 * dH_{i-1} = r16(W_i)^T dZ_i in fp32; dZ_{i-1} = r16(dH_{i-1}) where h_{i-1} is not <= 0 (the mask on the ROUNDED activation), else 0;
 * grad_x = dH_0 in fp32; dW_i = sum over the points of dZ_i (x) h_{i-1} (every product exact in fp32, summed in fp32 per workgroup and in
 * fp64 over the workgroups); db_i = sum of dZ_i in fp64.  The weights are converted from the caller's fp32 copy inside the kernels, on
 * every call.  The order of the terms inside one 32-wide block of a sum is the matrix instruction's; the blocks are added in index order.
 * A grad_y beyond fp16's range (a loss scale that is too large) becomes inf and reaches the gradients: the caller's grad scaler sees it.
 * Any other value of precision is SN_ERR_INVALID from sn_mlp_forward and sn_mlp_backward (sn_mlp_backward_workspace_bytes answers 0).
 * A library built before the field existed IGNORES it (it was `reserved`, read by no code) and computes in fp32; SN_MLP_ABI_VERSION cannot
 * tell the two apart, because no signature and no layout changed.  sn_train_normals_analytic ignores the field: it reads the weights in fp32.
 *
 * N >= 0; N == 0 returns SN_OK without a launch and without looking at the data pointers.  A NULL or unknown-size descriptor, n_layers or a
 * dimension outside its range, N < 0, N >= 2^31, a NULL required pointer and a workspace that is too small are SN_ERR_INVALID before the
 * device is touched.
 *
 * Versioning: SN_MLP_ABI_VERSION / sn_mlp_abi_version() version THIS header's signatures; SnMlpDesc is versioned by its struct_size
 * (signerf_hip.h "ABI evolution").
 */
#ifndef SIGNERF_HIP_MLP_H
#define SIGNERF_HIP_MLP_H

#include "signerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_MLP_ABI_VERSION 1
#define SN_MLP_MAX_LAYERS 4
#define SN_MLP_MAX_DIM 64
#define SN_MLP_PRECISION_FP32 0
#define SN_MLP_PRECISION_FP16 1
int sn_mlp_abi_version(void);

typedef struct SnMlpDesc {
    uint32_t struct_size;                    /* sizeof(SnMlpDesc) as the caller compiled it */
    int32_t n_layers;
    int32_t dims[SN_MLP_MAX_LAYERS + 1];     /* dims[0] = input width ... dims[n_layers] = output width */
    int32_t precision;                       /* SN_MLP_PRECISION_FP32 (0) or SN_MLP_PRECISION_FP16; the slot was `reserved`, 0, before */
    const float* weights[SN_MLP_MAX_LAYERS]; /* DEVICE [dims[i+1], dims[i]], the first n_layers are read */
    const float* biases[SN_MLP_MAX_LAYERS];  /* DEVICE [dims[i+1]] */
    /* sn_mlp_backward only: all of the first n_layers entries of BOTH arrays set, or all of them NULL (no weight gradients) */
    float* grad_weights[SN_MLP_MAX_LAYERS];  /* DEVICE [dims[i+1], dims[i]] */
    float* grad_biases[SN_MLP_MAX_LAYERS];   /* DEVICE [dims[i+1]] */
} SnMlpDesc;

/* y [N, dims[n_layers]] = the network of x [N, dims[0]].  The gradient pointers of the descriptor are ignored. */
int sn_mlp_forward(const SnMlpDesc* desc, const float* x, int64_t N, float* y, SnStream stream);

/* Bytes of workspace sn_mlp_backward needs to form the weight gradients of N points: one partial image of every dW_i and db_i per
 * workgroup, min(ceil(N / 64), 256) of them -- a function of N and the dims alone, never of the device.  Monotone in N.  0 for N <= 0 or
 * an invalid descriptor. */
size_t sn_mlp_backward_workspace_bytes(const SnMlpDesc* desc, int64_t N);

/* Backward of the above for the incoming grad_y [N, dims[n_layers]].  The hidden activations are recomputed from x: nothing but x itself
 * needs to be kept between the passes.
 *   grad_x [N, dims[0]]:        WRITTEN; may be NULL.
 *   desc->grad_weights[i], desc->grad_biases[i]: WRITTEN, NOT accumulated into -- dW_i = dZ_i^T H_{i-1}, db_i = sum over the points of dZ_i.
 *                               Every workgroup sums its points in registers and writes one partial image to the workspace; a second
 *                               kernel adds the partials in index order and OWNS these outputs (a caller that keeps a running sum adds
 *                               them itself).  NULL as a group: then workspace may be NULL too.  Not both grad_x and the group NULL.
 *   workspace: DEVICE, 4-byte aligned, at least sn_mlp_backward_workspace_bytes(desc, N) bytes when the weight gradients are asked for.
 * There are no float atomics: two calls on the same inputs give the same bits in every output.
 * N == 0: nothing is launched and NO output is touched -- grad_weights and grad_biases keep what they held (a caller that wants the
 * empty sum there writes the zeros itself, as signerf_amd/mlp.py does). */
int sn_mlp_backward(const SnMlpDesc* desc, const float* x, const float* grad_y, int64_t N, float* grad_x, void* workspace,
                    size_t workspace_bytes, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_MLP_H */
