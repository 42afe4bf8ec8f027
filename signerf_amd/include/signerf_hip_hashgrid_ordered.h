/*
 * signerf_hip_hashgrid_ordered.h -- companion header of signerf_hip_hashgrid.h and signerf_hip_hashgrid_tcnn.h: the ORDERED form of the
 * trainable grids' table gradient.  The backward entry points of those two headers sum grad_table with fp32 atomic adds, whose arrival
 * order is the device's; the two entry points here compute the same gradient without a float atomic: every contribution is stored once,
 * (row, contribution id) is sorted per level, and every row's list is summed in fp64 in ascending id order.  Opt-in: nothing in the
 * sibling headers changes.  It ships with the Python package (signerf_amd/include/, signerf_amd._lib.EXTENSIONS).  Exported from the
 * same libsignerf_hip.so; int status, sn_last_error(NULL) text, caller-owned device memory, work enqueued on the caller's stream, no
 * hidden sync, no handle.  DESIGN.md section 4 "Ordered table gradient".
 *
 * Tensors, ranges, alignment, the domain and the cells are the sibling's: sn_hashgrid_ordered_backward is sn_hashgrid_backward's grid
 * (nerfstudio's torch path), sn_hashgrid_ordered_tcnn_backward is sn_hashgrid_tcnn_backward's (tiny-cuda-nn's).
 *
 * Contract of grad_table.  For table element (r, f) the contributions are c = w_k * grad_enc[n, l, f] over every in-domain point n and
 * corner slot k whose row is r; w_k = wx wy wz is formed in fp64 from the fp32 offsets and the product is rounded to fp32 once, exactly as
 * the atomic form does.  Contribution (n, k) has the id 8 n + k.  S[r][f] is the sum of the row's contributions in fp64, taken in an order
 * that is a function of the number of contributions of the row alone, over the list in ascending id:
 *   up to 16 contributions: one after another;
 *   more: 64 partial sums, partial j over the list's entries j, j + 64, j + 128 ... one after another, then folded as
 *   p[j] += p[j + d] for d = 32, 16, 8, 4, 2, 1 (j < d).
 * grad_table[r][f] = fl32((double)grad_table[r][f] + S[r][f]): ACCUMULATED INTO, rounded once.  A row without a contribution is not
 * written.  A point outside the domain contributes nothing.
 *   |error| <= (2 + n 2^-29) 2^-24 A per element per call, n contributions, A = sum w |grad_enc|.
 * Bitwise reproducible: repeated calls, calls on other streams and calls beside other work give the same bits; nothing in the environment
 * (SN_HASHGRID_MERGE_MAX_SCALE included) is read.  No float atomic is issued; the only atomics are LDS integer counters of a histogram,
 * whose totals do not depend on arrival order.
 *
 * grad_q is the sibling's, by the same kernel: bit for bit what the atomic entry point returns.
 *
 * Workspace: DEVICE memory, 16-byte aligned, of at least sn_hashgrid_ordered_workspace_bytes(N, L, log2_T, F) bytes; required when
 * grad_table is given, ignored (may be NULL) when only grad_q is.  The levels are processed one after another in it, so its size does not
 * grow with L: 8 N (4 F + 16) bytes and a few counters.  Its contents after the call are unspecified.
 *
 * With grad_table, N >= 2^28 is SN_ERR_INVALID: the 8 N contribution ids of a level are 32-bit.  Split a larger batch and accumulate.
 * (A grad_q-only call forms no ids and takes N up to 2^31 - 1, like the sibling.)
 * N == 0 returns SN_OK without a launch and without looking at the pointers.  A NULL required pointer, a value outside the sibling's
 * ranges, a misaligned tensor or workspace, a workspace that is too small and L * T * F >= 2^31 are SN_ERR_INVALID before the device is
 * touched.
 *
 * Versioning: SN_HASHGRID_ORDERED_ABI_VERSION / sn_hashgrid_ordered_abi_version() version THIS header's signatures.
 */
#ifndef SIGNERF_HIP_HASHGRID_ORDERED_H
#define SIGNERF_HIP_HASHGRID_ORDERED_H

#include "../../include/signerf_hip.h" /* this header lives in signerf_amd/include/, the core header in the tree's include/ */

#ifdef __cplusplus
extern "C" {
#endif

#define SN_HASHGRID_ORDERED_ABI_VERSION 1
#define SN_HASHGRID_ORDERED_MAX_POINTS 268435455 /* 2^28 - 1 */
int sn_hashgrid_ordered_abi_version(void);

/* HOST only.  A function of its four arguments alone (never of the device), monotone in N; 0 for N <= 0, N >= 2^28 or any argument the
 * backward entry points refuse. */
size_t sn_hashgrid_ordered_workspace_bytes(int64_t N, int32_t L, int32_t log2_T, int32_t F);

/* sn_hashgrid_backward with the ordered table gradient.  grad_table [L*T,F] ACCUMULATED INTO, grad_q [N,3] written; either may be NULL,
 * not both; table may be NULL when grad_q is. */
int sn_hashgrid_ordered_backward(const float* q, const float* table, const float* scalings, const float* grad_enc, int64_t N, int32_t L,
                                 int32_t log2_T, int32_t F, float* grad_table, float* grad_q, void* workspace, size_t workspace_bytes,
                                 SnStream stream);

/* sn_hashgrid_tcnn_backward with the ordered table gradient. */
int sn_hashgrid_ordered_tcnn_backward(const float* q, const float* table, const float* scalings, const float* grad_enc, int64_t N, int32_t L,
                                      int32_t log2_T, int32_t F, float* grad_table, float* grad_q, void* workspace, size_t workspace_bytes,
                                      SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_HASHGRID_ORDERED_H */
