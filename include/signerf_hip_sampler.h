/*
 * signerf_hip_sampler.h -- companion header of signerf_hip.h: training-mode proposal sampling.  nerfstudio's SpacedSampler and PDFSampler
 * in their TRAINING branch (stratified jitter; include_original = False) together with the per-sample quantities a RaySamples carries:
 * Euclidean bins, deltas, positions and the fields' normalised positions.  The formulas are restated in DESIGN.md section 4
 * "Training-mode sampling".  Exported from the same libsignerf_hip.so and following the conventions of signerf_hip.h (int status,
 * sn_last_error(NULL) text, caller-owned device memory, work enqueued on the caller's stream, no hidden sync); no handle is needed.
 * The eval-mode stage entry point sn_pdf_sample of signerf_hip.h is a different one and is not touched by this header.
 *
 * Common to both entry points: all tensors are DEVICE memory, row-major and dense, fp32 but for selector (uint8).  One wave works on one
 * ray; the cdf's running sum is fp64; there are no atomics and no state shared between rays, so two calls on the same inputs give the
 * same bits and a non-finite near, far, origin or weight changes its own ray's rows only.  Both kernels terminate whatever the data.
 * n_rays >= 0; n_rays == 0 returns SN_OK without a launch and without looking at the pointers.  A negative n_rays, n_rays >= 2^31, a
 * sample count outside 1..SN_SAMPLER_MAX_SAMPLES, a NULL required pointer, a struct_size smaller than the first version of the struct
 * (or larger than the library's) and an anneal that is negative or not finite are SN_ERR_INVALID, decided before the device is touched.
 *
 * Random numbers.  With rand == NULL the kernels draw from Philox4x32-10: key (seed_lo, seed_hi), counter (ray, j, offset_lo, offset_hi)
 * with j the index of the bin edge (0 under single_jitter), word 0 of the block, float = (x >> 8) * 2^-24 in [0, 1).  With rand != NULL
 * the caller's numbers are used instead: [n_rays] under single_jitter, else [n_rays, n_samples + 1].  rand_out (same layout, may be NULL)
 * receives the numbers actually used; a seeded call and a second call fed its rand_out give the same bits everywhere.
 *
 * Versioning: SN_SAMPLER_ABI_VERSION / sn_sampler_abi_version() version THIS header's signatures; the structs grow at the end and begin
 * with struct_size = sizeof(the struct) in the caller's header (signerf_hip.h "ABI evolution").
 */
#ifndef SIGNERF_HIP_SAMPLER_H
#define SIGNERF_HIP_SAMPLER_H

#include "signerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_SAMPLER_ABI_VERSION 1
#define SN_SAMPLER_MAX_SAMPLES 1024
int sn_sampler_abi_version(void);

/* The rays, the jitter and the outputs: what both samplers share. */
typedef struct SnSamplerRays {
    uint32_t struct_size;
    int32_t n_samples;        /* M: samples out, 1..SN_SAMPLER_MAX_SAMPLES */
    int64_t n_rays;           /* R */
    const float* origins;     /* [R,3] required */
    const float* directions;  /* [R,3] required */
    const float* nears;       /* [R] or NULL: near_plane for every ray */
    const float* fars;        /* [R] or NULL: far_plane for every ray */
    float near_plane;
    float far_plane;
    int32_t spacing_mode;     /* 0: s(x) of UniformLinDispPiecewiseSampler; 1: UniformSampler's identity */
    int32_t single_jitter;    /* non-zero: one uniform number per ray instead of one per bin edge */
    const float* rand;        /* see "Random numbers"; NULL: Philox */
    uint64_t seed;
    uint64_t offset;
    /* outputs; each may be NULL, and a NULL output is not computed */
    float* spacing_bins;      /* [R,M+1] bin edges in the normalised (spacing) domain */
    float* euclid_bins;       /* [R,M+1] s^-1(bins * s_far + (1 - bins) * s_near) */
    float* deltas;            /* [R,M]   e_{i+1} - e_i */
    float* positions;         /* [R,M,3] o + d * (e_i + e_{i+1}) / 2 */
    float* q;                 /* [R,M,3] contract_inf(position), (p + 2) / 4, multiplied by the selector */
    uint8_t* selector;        /* [R,M]   ((q > 0) & (q < 1)).all(-1) */
    float* rand_out;          /* the layout of rand */
} SnSamplerRays;

/* The PDF resampler's own inputs. */
typedef struct SnSamplerPdf {
    uint32_t struct_size;
    int32_t n_in;               /* N: intervals of the previous level, 1..SN_SAMPLER_MAX_SAMPLES */
    const float* spacing_bins;  /* [R,N+1] required: the previous level's spacing bins, non-decreasing along a ray */
    const float* weights;       /* [R,N]   required */
    const float* u_grid;        /* DEVICE [M+1] required: linspace(0, 1 - 1/(M+1), M+1) */
    float anneal;               /* w = pow(weights, anneal); the pow is skipped for 1; >= 0 and finite */
    float histogram_padding;
} SnSamplerPdf;

/* SpacedSampler, training branch.  base_bins: DEVICE [M+1], required (linspace(0, 1, M+1)).
 *   c_i = (b_{i+1} + b_i) / 2, upper = [c, b_M], lower = [b_0, c], bins = lower + (upper - lower) * t, t = rand[r] or rand[r, j];
 *   all of it un-fused fp32 in torch's operand order. */
int sn_sampler_initial(const SnSamplerRays* rays, const float* base_bins, SnStream stream);

/* PDFSampler, training branch, include_original = False.
 *   w = pow(weights, anneal) + histogram_padding, padded once more when its sum is below 1e-5 and normalised as sn_pdf_sample does,
 *   cdf = [0, min(1, cumsum(pdf))], u_j = u_grid[j] + rand / (M + 1), idx = searchsorted(cdf, u, right),
 *   t = clip(nan_to_num((u - c0) / (c1 - c0), 0), 0, 1), bin = b0 + t * (b1 - b0) with 0 / 1 the knots idx - 1 / idx clamped to [0, N].
 * The bins carry no gradient (nerfstudio detaches them). */
int sn_sampler_pdf(const SnSamplerRays* rays, const SnSamplerPdf* pdf, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_SAMPLER_H */
