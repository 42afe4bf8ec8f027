/*
 * signerf_hip_hashgrid_tcnn.h -- companion header of signerf_hip.h: the trainable tiny-cuda-nn grid.  The sibling of
 * signerf_hip_hashgrid.h for fields imported from an `ns-train nerfacto` checkpoint (signerf_amd/tcnn_import.py): the same three
 * kernels, the same conventions and the same CALLER-owned uniform table, with tiny-cuda-nn's cells instead of nerfstudio's torch-path
 * ones -- its own per-level scales, floor / floor + 1 corners and densely indexed coarse levels.  The semantics are those of
 * oracle/tcnn_layout.py (grid_meta, grid_rows, grid_encode), restated in DESIGN.md section 4 "Trainable tcnn grid"; like everything about
 * that library here they are UNPINNED against the library itself.  It ships with the Python package (signerf_amd/include/,
 * signerf_amd._lib.EXTENSIONS) beside the headers of the tree's include/.  Exported from the same libsignerf_hip.so; int status,
 * sn_last_error(NULL) text, caller-owned device memory, work enqueued on the caller's stream, no hidden sync, no handle.
 *
 * Common to forward and backward: all tensors are DEVICE memory, row-major and dense; fp32 but for idx (int32).
 *   q        [N,3]     the points (the field hands over q * selector in [0,1); every bit pattern is defined, see "Domain")
 *   table    [L*T,F]   T = 2^log2_T rows per level slot, level l at rows [l T, (l+1) T); a level of n_l < T rows uses the first n_l
 *   scalings [L]       DEVICE fp32, the library's grid_scale(): exp2f(l log2f(growth)) base - 1
 *   1 <= L <= SN_HASHGRID_TCNN_MAX_LEVELS, 1 <= log2_T <= SN_HASHGRID_TCNN_MAX_LOG2_T, F in {1, 2, 4, 8}.  L * T * F >= 2^31 is
 *   SN_ERR_INVALID: the kernels' element offsets into the table are 32-bit.  N >= 0; N == 0 returns SN_OK without a launch and without
 *   looking at the pointers.  A negative N, N >= 2^31, a value outside these ranges and a NULL required pointer are SN_ERR_INVALID.
 *   table, enc, grad_enc and grad_table must be aligned to min(4 F, 16) bytes and idx to 16.
 *
 * Semantics, per point and level l with s = scalings[l]:
 *   x = fmaf(s, q, 0.5) (one rounding), c = floor(x), w = x - c.
 *   Corner k = 0..7 adds 1 to c on axis a where bit a of k is set (x is axis 0); its weight is the product over the axes of w_a where the
 *   bit is set and 1 - w_a where it is clear.
 *   r = ceil(s) + 1, n = min(next_multiple(r^3, 8), T).  The level is DENSE iff r^3 <= n (so r <= 256): corner (x, y, z) reads row
 *   (x + y r + z r^2) in wrapping uint32, then % n -- a true modulo.  Otherwise it is HASHED: row ((x * 1) ^ (y * 2654435761) ^
 *   (z * 805459861)) in wrapping uint32, & (T - 1).  Both + l T.
 *   enc [N, L*F], level-major, is sum_k weight_k table[row_k], summed in fp32 from corner 0 up, the weight formed as ((1 wx) wy) wz.
 *
 * Domain.  A point is in domain iff x is finite and in [0, 2^30) on every axis at EVERY level.  (A negative x is undefined in the library:
 * it is refused, not guessed.)  Outside the domain the behaviour is signerf_hip_hashgrid.h's: every feature is NaN, the idx rows are 0,
 * the point adds NOTHING to grad_table and its grad_q row is NaN.  No input -- no scalings either -- addresses outside a level's slot.
 *
 * Reproducibility: enc, idx and grad_q have no shared state, two calls give the same bits.  grad_table is summed with fp32 atomic adds;
 * per element the error is bounded by (n + 4) 2^-24 sum |w g| for n contributions.  Rows of a dense slot beyond n_l get no contribution.
 *
 * Versioning: SN_HASHGRID_TCNN_ABI_VERSION / sn_hashgrid_tcnn_abi_version() version THIS header's signatures.
 */
#ifndef SIGNERF_HIP_HASHGRID_TCNN_H
#define SIGNERF_HIP_HASHGRID_TCNN_H

#include "../../include/signerf_hip.h" /* this header lives in signerf_amd/include/, the core header in the tree's include/ */

#ifdef __cplusplus
extern "C" {
#endif

#define SN_HASHGRID_TCNN_ABI_VERSION 1
#define SN_HASHGRID_TCNN_MAX_LEVELS 32
#define SN_HASHGRID_TCNN_MAX_LOG2_T 24
int sn_hashgrid_tcnn_abi_version(void);

/* HOST only, no device is touched: the geometry of every level as the kernels derive it, from HOST scalings [L].  res[l] = r, rows[l] =
 * n, dense[l] = 1 or 0; each of the three may be NULL.  The same definition the kernels compile (csrc/sn_hashgrid_tcnn.h, sn_tcnn_level). */
int sn_hashgrid_tcnn_levels(const float* scalings, int32_t L, int32_t log2_T, int32_t* res, int32_t* rows, int32_t* dense);

/* enc [N, L*F]: required.  idx [N,L,8] int32, the row (with its level's offset l T) of every corner in the order above: may be NULL. */
int sn_hashgrid_tcnn_forward(const float* q, const float* table, const float* scalings, int64_t N, int32_t L, int32_t log2_T, int32_t F,
                             float* enc, int32_t* idx, SnStream stream);

/* Backward of the above for the incoming grad_enc [N, L*F]; indices and weights are recomputed from q.
 *   grad_table [L*T,F]: ACCUMULATED INTO: grad_table[row_k] += weight_k grad_enc, the product formed in fp64 and rounded once.
 *   grad_q     [N,3]:   written: grad_q_a = sum_l scalings[l] sum_f grad_enc d enc / d w_a, fp64 sums rounded once.
 *   Either may be NULL, not both; table may be NULL when grad_q is.  scalings get no gradient.
 * The two forms of grad_table's atomics and their switch are the sibling's (SN_HASHGRID_MERGE_MAX_SCALE, sn_hashgrid_debug_reload_env);
 * without the variable this grid merges the levels with scale <= its own shipped threshold. */
int sn_hashgrid_tcnn_backward(const float* q, const float* table, const float* scalings, const float* grad_enc, int64_t N, int32_t L,
                              int32_t log2_T, int32_t F, float* grad_table, float* grad_q, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_HASHGRID_TCNN_H */
