/*
 * signerf_hip_hashgrid.h -- companion header of signerf_hip.h: the trainable hash grid.  nerfstudio's torch-path HashEncoding (SURVEY.md
 * A7, restated in oracle.nerfacto.hash_corner_indices / hash_encode) on a table the CALLER owns -- a torch Parameter -- with a forward and
 * a backward entry point.  It is the one piece of a nerfacto field that plain torch ops do badly (8 L scattered rows per point, an
 * index_add over 8 L N rows backwards); the MLPs, the SH encoding and trunc_exp around it stay torch ops.  The formulas are restated in
 * DESIGN.md section 4 "Trainable hash grid".  Exported from the same libsignerf_hip.so and following the conventions of signerf_hip.h (int
 * status, sn_last_error(NULL) text, caller-owned device memory, work enqueued on the caller's stream, no hidden sync); no handle is needed.
 * sn_hash_encode of signerf_hip.h (the handle's uploaded tables, eval only) is a different entry point and is not touched by this one.
 *
 * Common to both entry points: all tensors are DEVICE memory, row-major and dense; fp32 but for idx (int32).
 *   q        [N,3]     the points (the field hands over positions in [0,1]; every bit pattern is defined, see "Domain")
 *   table    [L*T,F]   T = 2^log2_T rows per level, level l at rows [l T, (l+1) T)
 *   scalings [L]       DEVICE fp32, the per-level grid scale (floor(base * growth^l) in nerfstudio)
 *   1 <= L <= SN_HASHGRID_MAX_LEVELS, 1 <= log2_T <= SN_HASHGRID_MAX_LOG2_T, F in {1, 2, 4, 8}.  L * T * F >= 2^31 (an 8 GiB table) is
 *   SN_ERR_INVALID: the kernels' element offsets into the table are 32-bit.  N >= 0; N == 0 returns SN_OK without a launch and without
 *   looking at the pointers (an empty tensor's may be NULL).  A negative N, N >= 2^31, a value outside these ranges and a NULL required
 *   pointer are SN_ERR_INVALID.  table, enc, grad_enc and grad_table must be aligned to min(4 F, 16) bytes and idx to 16 (rows are moved
 *   with one vector access); any allocation of a HIP allocator is.
 *
 * Semantics, per point and level l: scaled = q * scalings[l] (one IEEE fp32 multiply), floor and ceil to int32, offset o = scaled - floor.
 * Corner k = 0..7 takes ceil (c) or floor (f) per axis in nerfstudio's order 0 ccc, 1 cfc, 2 ffc, 3 fcc, 4 ccf, 5 cff, 6 fff, 7 fcf
 * (x y z) and reads row ((x * 1) ^ (y * 2654435761) ^ (z * 805459861)) mod T + l T -- every level is hashed; wrapping uint32 products
 * and "& (T - 1)" give torch's int64 result for every int32 coordinate.  The blend is nerfstudio's nesting in fp32,
 *   f03 = f0 ox + f3 (1 - ox), f12 = f1 ox + f2 (1 - ox), f56 = f5 ox + f6 (1 - ox), f47 = f4 ox + f7 (1 - ox),
 *   f0312 = f03 oy + f12 (1 - oy), f4756 = f47 oy + f56 (1 - oy), enc = f0312 oz + f4756 (1 - oz),
 * and the output is level-major, enc [N, L*F].  A point on a lattice plane has floor = ceil on that axis: both corners are the same row
 * and carry the weights o = 0 and 1 - o = 1, as autograd has it.
 *
 * Domain -- a deliberate deviation from torch.  A point with a non-finite coordinate, or with |q_a * scalings[l]| >= 2^30 for any axis a
 * and ANY level l, is out of domain (in torch the cast of such a value to int32 is undefined and poisons whichever rows it picks).  For
 * such a point every feature is NaN, its idx rows are 0, it adds NOTHING to grad_table and its grad_q row is NaN.  The row index is
 * masked with T - 1, so no input can address outside the table.
 *
 * Reproducibility.  enc, idx and grad_q have no shared state: two calls on the same inputs give the same bits.  grad_table is summed with
 * fp32 atomic adds, because table rows are shared across the whole batch: two calls may differ in the last bits (the sum's order is the
 * arrival order).  Per element the error is bounded by (n + 4) 2^-24 sum |w g| for n contributions.
 *
 * Versioning: SN_HASHGRID_ABI_VERSION / sn_hashgrid_abi_version() version THIS header's signatures.
 */
#ifndef SIGNERF_HIP_HASHGRID_H
#define SIGNERF_HIP_HASHGRID_H

#include "signerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_HASHGRID_ABI_VERSION 1
#define SN_HASHGRID_MAX_LEVELS 32
#define SN_HASHGRID_MAX_LOG2_T 24
int sn_hashgrid_abi_version(void);

/* enc [N, L*F]: required.  idx [N,L,8] int32, the row (with its level's offset l T) of every corner in the order above: may be NULL. */
int sn_hashgrid_forward(const float* q, const float* table, const float* scalings, int64_t N, int32_t L, int32_t log2_T, int32_t F,
                        float* enc, int32_t* idx, SnStream stream);

/* Backward of the above for the incoming grad_enc [N, L*F].  Indices and weights are recomputed from q: nothing but q itself needs to be
 * kept between the passes.
 *   grad_table [L*T,F]: ACCUMULATED INTO -- the caller zeroes it (or keeps a running sum in it):
 *                       grad_table[row_k] += wx wy wz grad_enc, the corner's three weights (o or 1 - o per axis), each product in [0,1].
 *   grad_q     [N,3]:   written: grad_q_a = sum_l scalings[l] sum_f grad_enc d enc / d o_a, the literal derivative of the blend, e.g.
 *                       d/d ox = [(f0 - f3) oy + (f1 - f2)(1 - oy)] oz + [(f4 - f7) oy + (f5 - f6)(1 - oy)] (1 - oz).
 *   Either may be NULL, not both; table may be NULL when grad_q is.  scalings get no gradient. */
int sn_hashgrid_backward(const float* q, const float* table, const float* scalings, const float* grad_enc, int64_t N, int32_t L,
                         int32_t log2_T, int32_t F, float* grad_table, float* grad_q, SnStream stream);

/* Diagnostic.  grad_table's atomics have two forms: one add per corner and feature, and -- for the levels whose scale is at most a
 * threshold -- a form that first sums, within a wave, the lanes that follow each other with the same row (consecutive samples of a ray
 * share cells on a coarse level).  Both meet the bound above.  The threshold is read from the environment (SN_HASHGRID_MERGE_MAX_SCALE; a
 * negative value: no level merges) by the first backward call of the process; this re-reads it, for A/B measurements. */
int sn_hashgrid_debug_reload_env(void);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_HASHGRID_H */
