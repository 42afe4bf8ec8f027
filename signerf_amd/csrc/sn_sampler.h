// sn_sampler.h -- training-mode proposal sampling (include/signerf_hip_sampler.h): nerfstudio's SpacedSampler and PDFSampler in their
// TRAINING branch (stratified jitter, include_original=False) [NS-RECALL, nerfstudio 1.0.2 model_components/ray_samplers.py], and the
// per-sample quantities a RaySamples carries.  The formulas are restated in DESIGN.md §4 "Training-mode sampling";
// tests/sampler_oracle.py holds them as plain torch ops.
//
// Mapping: ONE WAVE PER RAY, as in sn_losses.h.  64-thread blocks, block r works on ray r; lane l takes the elements l, l + 64, ... of the
// row-major rows, so every load and store of a row is coalesced.  (sn_pdf_stage_kernel of sn_proposal.h is one ray per lane on row-major
// rows: every access strides by a row.  Its mapping is not reused.)
//   pdf kernel:  pass 1  w' = pow(w, anneal) -> LDS;  w' + pad summed in fp64 (a butterfly) -> SnPdfNorm
//                pass 2  pdf_i in strict fp32, its running sum a wave scan in fp64 with a chunk carry, rounded to the fp32 knots
//                        min(1, .) with a leading 0 -> LDS, beside the ray's existing bins
//                pass 3  lane takes the outputs j = lane, lane + 64, ...: u_j, ONE binary search in the LDS knots (at most 11 steps for
//                        N <= 1024, bounded for any data: the interval halves whatever the compares say), interpolation, the Euclidean
//                        map; the new Euclidean bins go to LDS
//                pass 4  lane i reads Euclidean bins i and i + 1: deltas, positions, q, selector
//   initial kernel: passes 3 (the jittered grid instead of the search) and 4.
// Only dynamic LDS, sized per launch (sn_sampler_lds_*).  No atomics and no state shared between rays: two calls give the same bits, and a
// non-finite value stays in its own ray.  Loops that hold a shuffle run a wave-uniform number of times (lanes past N carry zeros).
//
// Arithmetic: everything that reaches an output is un-fused IEEE fp32 in torch's operand order, but for the cdf, which torch.cumsum forms
// from fp32 data; here it is accumulated in fp64 and rounded once per knot (sn_device.h "Numerics contract").
#pragma once
#include "sn_device.h"
#include "sn_losses.h"
#include "sn_proposal.h"

#define SN_SAMPLER_MAX_S 1024   // samples per ray, in and out: the loss kernels' limit

struct SnSamplerParams {
    // rays
    const float* origins;      // [R,3]
    const float* directions;   // [R,3]
    const float* nears;        // [R] or nullptr: near_plane
    const float* fars;         // [R] or nullptr: far_plane
    float near_plane, far_plane;
    int spacing_uniform;   // 0 piecewise, 1 uniform (sn_spacing)
    int single_jitter;
    const float* rand;     // [R] (single jitter) or [R,M+1]; nullptr: Philox
    uint64_t seed, offset;
    const float* grid;     // initial: the base bins b [M+1]; pdf: the u grid g [M+1]
    int M;                 // samples out
    // pdf only
    const float* sbins;     // [R,N+1]
    const float* weights;   // [R,N]
    int N;
    float anneal, hist_pad;
    // outputs, each may be nullptr
    float* spacing_bins;   // [R,M+1]
    float* euclid_bins;    // [R,M+1]
    float* deltas;         // [R,M]
    float* positions;      // [R,M,3]
    float* q;              // [R,M,3]
    uint8_t* selector;     // [R,M]
    float* rand_out;       // the layout of rand
};

static inline size_t sn_sampler_lds_initial(int M) { return (size_t)(M + 1) * 4; }
static inline size_t sn_sampler_lds_pdf(int N, int M) { return (size_t)(N + 1) * 8 + (size_t)(M + 1) * 4; }

// ---- Philox4x32-10 (Salmon et al., SC'11; Random123's constants): word 0 of the block for counter (c0, c1, c2, c3) and key (k0, k1) ---------
SN_DEV uint32_t sn_philox4x32_10_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// the uniform number of (ray, j): the caller's, or (x >> 8) 2^-24 in [0, 1)
SN_DEV float sn_sampler_rand(const SnSamplerParams& p, int j) {
    const int jj = p.single_jitter ? 0 : j;
    if (p.rand) return p.rand[p.single_jitter ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (p.M + 1) + jj];
    const uint32_t x = sn_philox4x32_10_word0(blockIdx.x, (uint32_t)jj, (uint32_t)p.offset, (uint32_t)(p.offset >> 32), (uint32_t)p.seed,
                                              (uint32_t)(p.seed >> 32));
    return (float)(x >> 8) * 0x1p-24f;
}

SN_DEV void sn_sampler_rand_out(const SnSamplerParams& p, int j, float t) {
    if (!p.rand_out) return;
    if (!p.single_jitter) p.rand_out[(int64_t)blockIdx.x * (p.M + 1) + j] = t;
    else if (j == 0) p.rand_out[blockIdx.x] = t;
}

// Frustums.get_positions, SceneContraction(inf), (p + 2) / 4 and the fields' selector, literally: torch's inf-norm hands a NaN coordinate
// on (fmaxf would skip it) and the selector is the six compares (a NaN fails them).
SN_DEV bool sn_sampler_q(const float o[3], const float d[3], float start, float end, float pos[3], float q[3]) {
#pragma clang fp contract(off)
    const float t = start + end;
    float p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[c] = p[c] = o[c] + (d[c] * t) / 2.0f;
    float mag = fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2]));
    if (p[0] != p[0] || p[1] != p[1] || p[2] != p[2]) mag = __builtin_nanf("");
    if (!(mag < 1.0f)) {
        const float k = 2.0f - (1.0f / mag);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = k * (p[c] / mag);
    }
    bool sel = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q[c] = (p[c] + 2.0f) / 4.0f;
        sel = sel && q[c] > 0.0f && q[c] < 1.0f;
    }
    const float m = sel ? 1.0f : 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = q[c] * m;
    return sel;
}

// pass 4: eb [M+1] in LDS holds the ray's Euclidean bins (the barrier behind its last write is the caller's)
SN_DEV void sn_sampler_emit_samples(const SnSamplerParams& p, const float* eb) {
    if (!p.deltas && !p.positions && !p.q && !p.selector) return;
    const int lane = threadIdx.x, M = p.M;
    const int64_t row = (int64_t)blockIdx.x * M;
    float o[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = p.origins[(int64_t)blockIdx.x * 3 + c];
        d[c] = p.directions[(int64_t)blockIdx.x * 3 + c];
    }
    for (int i = lane; i < M; i += 64) {
        const float e0 = eb[i], e1 = eb[i + 1];
        if (p.deltas) {
#pragma clang fp contract(off)
            p.deltas[row + i] = e1 - e0;
        }
        if (p.positions || p.q || p.selector) {
            float pos[3], q[3];
            const bool sel = sn_sampler_q(o, d, e0, e1, pos, q);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (p.positions) p.positions[(row + i) * 3 + c] = pos[c];
                if (p.q) p.q[(row + i) * 3 + c] = q[c];
            }
            if (p.selector) p.selector[row + i] = sel ? 1 : 0;
        }
    }
}

extern __shared__ __attribute__((aligned(16))) unsigned char sn_sampler_lds[];

// ---- SpacedSampler, training branch ----------------------------------------------------------------------------------------------------------
//   c_i = (b_{i+1} + b_i) / 2, upper = [c, b_M], lower = [b_0, c], bins = lower + (upper - lower) t,  t = rand[r] or rand[r, j]
//   euclid = s^-1(bins s_far + (1 - bins) s_near)
__global__ __launch_bounds__(64) void sn_train_sampler_initial_kernel(SnSamplerParams p) {
    const int lane = threadIdx.x, M = p.M;
    float* eb = (float*)sn_sampler_lds;   // [M+1]
    const int su = p.spacing_uniform;
    const float s_near = sn_spacing(p.nears ? p.nears[blockIdx.x] : p.near_plane, su);
    const float s_far = sn_spacing(p.fars ? p.fars[blockIdx.x] : p.far_plane, su);
    const int64_t brow = (int64_t)blockIdx.x * (M + 1);
    for (int j = lane; j <= M; j += 64) {
        const float t = sn_sampler_rand(p, j);
        sn_sampler_rand_out(p, j, t);
        float bin;
        {
#pragma clang fp contract(off)
            const float bj = p.grid[j];
            const float lower = j == 0 ? bj : (bj + p.grid[j - 1]) / 2.0f;
            const float upper = j == M ? bj : (p.grid[j + 1] + bj) / 2.0f;
            bin = lower + (upper - lower) * t;
        }
        const float e = sn_euclid(bin, s_near, s_far, su);
        eb[j] = e;
        if (p.spacing_bins) p.spacing_bins[brow + j] = bin;
        if (p.euclid_bins) p.euclid_bins[brow + j] = e;
    }
    __syncthreads();
    sn_sampler_emit_samples(p, eb);
}

// ---- PDFSampler, training branch, include_original = False -----------------------------------------------------------------------------------
//   w = pow(weights, anneal) (skipped for anneal == 1), padding and normalisation as SnPdfNorm (oracle.nerfacto.pdf_sample),
//   cdf = [0, min(1, cumsum(pdf))],  u_j = g_j + rand / (M + 1),  idx = searchsorted(cdf, u, right),
//   t = clip(nan_to_num((u - c0) / (c1 - c0), 0), 0, 1),  bin = b0 + t (b1 - b0)   with 0 / 1 the knots idx - 1 / idx clamped to [0, N]
__global__ __launch_bounds__(64) void sn_train_sampler_pdf_kernel(SnSamplerParams p) {
    const int lane = threadIdx.x, N = p.N, M = p.M;
    float* cdf = (float*)sn_sampler_lds;   // [N+1]
    float* sb = cdf + (N + 1);             // [N+1]
    float* eb = sb + (N + 1);              // [M+1]
    const float* w = p.weights + (int64_t)blockIdx.x * N;
    const float* sbin = p.sbins + (int64_t)blockIdx.x * (N + 1);
    const bool annealed = p.anneal != 1.0f;
    // pass 1: the sum of the padded weights; the annealed weight waits in the slot of its own knot (the same lane comes back for it)
    double swp = 0.0;
    for (int i = lane; i < N; i += 64) {
#pragma clang fp contract(off)
        const float wi = annealed ? powf(w[i], p.anneal) : w[i];
        cdf[i + 1] = wi;
        swp += (double)(wi + p.hist_pad);
    }
    swp = sn_loss_wave_sum(swp);
    SnPdfNorm nm;
    nm.set(swp, N);
    // pass 2: the knots
    double carry = 0.0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        float pdf = 0.0f;
        if (i < N) {
#pragma clang fp contract(off)
            pdf = ((cdf[i + 1] + p.hist_pad) + nm.padding) / nm.denom;
        }
        const double incl = sn_loss_scan_up((double)pdf, lane) + carry;
        carry = __shfl(incl, 63, 64);
        if (i < N) cdf[i + 1] = fminf(1.0f, (float)incl);
    }
    for (int i = lane; i <= N; i += 64) sb[i] = sbin[i];
    if (lane == 0) cdf[0] = 0.0f;
    __syncthreads();
    // pass 3: the new bins
    const int su = p.spacing_uniform;
    const float s_near = sn_spacing(p.nears ? p.nears[blockIdx.x] : p.near_plane, su);
    const float s_far = sn_spacing(p.fars ? p.fars[blockIdx.x] : p.far_plane, su);
    const int64_t brow = (int64_t)blockIdx.x * (M + 1);
    for (int j = lane; j <= M; j += 64) {
        const float r = sn_sampler_rand(p, j);
        sn_sampler_rand_out(p, j, r);
        float bin;
        {
#pragma clang fp contract(off)
            const float u = p.grid[j] + r / (float)(M + 1);
            const int idx = sn_loss_count_le(cdf, N + 1, u);
            const int below = min(max(idx - 1, 0), N), above = min(max(idx, 0), N);
            const float c0 = cdf[below], c1 = cdf[above], b0 = sb[below], b1 = sb[above];
            float t = (u - c0) / (c1 - c0);
            if (t != t) t = 0.0f;
            t = fminf(fmaxf(t, 0.0f), 1.0f);
            bin = b0 + t * (b1 - b0);
        }
        const float e = sn_euclid(bin, s_near, s_far, su);
        eb[j] = e;
        if (p.spacing_bins) p.spacing_bins[brow + j] = bin;
        if (p.euclid_bins) p.euclid_bins[brow + j] = e;
    }
    __syncthreads();
    sn_sampler_emit_samples(p, eb);
}
