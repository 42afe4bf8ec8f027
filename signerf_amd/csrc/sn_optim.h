// sn_optim.h -- kernels of include/signerf_hip_optim.h: the fused Adam step (DESIGN.md §4 "Optimiser step").  Three kinds of launch on one
// stream, each taking up to kSnAdamMaxTensors tensors as kernel arguments (SnAdamArgs; sn_optim_plan.h says which workgroup works where):
//   sn_optim_adam_stats_kernel     one fp64 sum of squares per chunk of a clipping group's gradients, to the workspace (no atomics)
//   sn_optim_adam_prologue_kernel  one workgroup per tensor: sums its group's partials in a fixed order, then ONE lane advances `step`
//                                  and writes the tensor's record (skip, s, lr / bc1, sqrt(bc2), norm_G) -- so no workgroup of the
//                                  update races a write of `step`
//   sn_optim_adam_update_kernel    the elementwise step, 16-byte accesses where the tensor's four pointers allow, scalar ones elsewhere
//                                  and always on the last n % 4 elements
// (The names are longer than 23 characters: DESIGN.md §4 "Wide fields", "Kernel names".)
#pragma once

#include "sn_optim_plan.h"

struct SnAdamArgs {
    float* param[kSnAdamMaxTensors];
    const float* grad[kSnAdamMaxTensors];
    float* exp_avg[kSnAdamMaxTensors];
    float* exp_avg_sq[kSnAdamMaxTensors];
    float* step[kSnAdamMaxTensors];
    int64_t n[kSnAdamMaxTensors];
    uint32_t prefix[kSnAdamMaxTensors + 1];  // SnAdamBatch::prefix
    uint32_t record[kSnAdamMaxTensors];      // the tensor's record = its index in the caller's array
    uint32_t part_own[kSnAdamMaxTensors], part_lo[kSnAdamMaxTensors], part_hi[kSnAdamMaxTensors];  // SnAdamPlan, per slot
    float lr[kSnAdamMaxTensors], beta1[kSnAdamMaxTensors], beta2[kSnAdamMaxTensors], eps[kSnAdamMaxTensors], weight_decay[kSnAdamMaxTensors],
        max_norm[kSnAdamMaxTensors];
    uint32_t vector_mask;  // bit k: param, grad, exp_avg and exp_avg_sq of slot k are 16-byte aligned
    int32_t n_slots;
    uint32_t n_chunks;
    const float* grad_scale;
    const float* found_inf;
    SnAdamRecord* records;
    double* partials;
};
static_assert(sizeof(SnAdamArgs) <= 4096, "the descriptors travel as kernel arguments");
static_assert(sizeof(SnAdamRecord) == kSnAdamRecordBytes, "sn_optim_plan.h lays the workspace out");
static_assert(kSnAdamMaxTensors == SN_ADAM_MAX_TENSORS && kSnAdamMaxTensors <= 32, "vector_mask has a bit per slot");
static_assert(kSnAdamChunk == 4 * 4 * kSnAdamBlock, "a lane makes four 16-byte accesses per chunk");

// sum of 256 lanes' values in a fixed tree; the result is valid in lane 0.  Ends with the LDS free for the next call.
__device__ inline double sn_adam_block_sum(double x, double* sh) {
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int w = kSnAdamBlock / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kSnAdamBlock) void sn_optim_adam_stats_kernel(SnAdamArgs a) {
    __shared__ double sh[kSnAdamBlock];
    const int t = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const SnAdamChunkRef r = sn_adam_locate(a.prefix, a.n_slots, a.n, c);
        const int k = r.slot;
        if (a.part_lo[k] == a.part_hi[k]) continue;  // (uniform) its group does not clip
        const float* g = a.grad[k] + r.first;
        double acc = 0.0;
        if ((a.vector_mask >> k) & 1u) {
            const int whole = r.count & ~3;
            for (int i = 4 * t; i < whole; i += 4 * kSnAdamBlock) {
                const float4 q = *reinterpret_cast<const float4*>(g + i);
                acc += (double)q.x * (double)q.x;
                acc += (double)q.y * (double)q.y;
                acc += (double)q.z * (double)q.z;
                acc += (double)q.w * (double)q.w;
            }
            if (whole + t < r.count) acc += (double)g[whole + t] * (double)g[whole + t];
        } else {
            for (int i = t; i < r.count; i += kSnAdamBlock) acc += (double)g[i] * (double)g[i];
        }
        const double total = sn_adam_block_sum(acc, sh);
        if (t == 0) a.partials[a.part_own[k] + (c - a.prefix[k])] = total;
    }
}

// beta^e for an integer e >= 0 by squaring, fp64: at most 2 log2(e) roundings, far below the fp32 rounding that follows
__device__ inline double sn_adam_powi(double b, uint64_t e) {
    double r = 1.0;
    while (e) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

__global__ __launch_bounds__(kSnAdamBlock) void sn_optim_adam_prologue_kernel(SnAdamArgs a) {
#pragma clang fp contract(off)
    __shared__ double sh[kSnAdamBlock];
    const int k = blockIdx.x;
    if (k >= a.n_slots) return;
    double acc = 0.0;
    for (uint32_t i = a.part_lo[k] + threadIdx.x; i < a.part_hi[k]; i += kSnAdamBlock) acc += a.partials[i];
    const double sumsq = sn_adam_block_sum(acc, sh);
    if (threadIdx.x != 0) return;
    const bool skip = a.found_inf && *a.found_inf != 0.0f;
    const float scale = a.grad_scale ? *a.grad_scale : 1.0f;
    const float inv_scale = a.grad_scale ? __fdiv_rn(1.0f, scale) : 1.0f;
    const bool clips = a.part_lo[k] != a.part_hi[k];
    const double norm = clips ? __dsqrt_rn(sumsq) : 0.0;
    float clip = 1.0f;
    if (clips) {
        const double c = (double)a.max_norm[k] / (norm / (double)scale + 1e-6);
        clip = (float)(c > 1.0 ? 1.0 : c);  // (a NaN stays a NaN, as torch's clamp keeps it)
    }
    const float t = *a.step[k] + 1.0f;
    if (!skip) *a.step[k] = t;
    const uint64_t e = t >= 1.0f ? (t < 1.0e12f ? (uint64_t)t : (uint64_t)1.0e12f) : 0ull;  // (beta < 1 in fp32: beta^1e12 is 0 already)
    const double bc1 = 1.0 - sn_adam_powi((double)a.beta1[k], e), bc2 = 1.0 - sn_adam_powi((double)a.beta2[k], e);
    SnAdamRecord rec;
    rec.skip = skip ? 1u : 0u;
    rec.grad_multiplier = __fmul_rn(inv_scale, clip);
    rec.step_size = (float)((double)a.lr[k] / bc1);
    rec.sqrt_bc2 = (float)__dsqrt_rn(bc2);
    rec.grad_norm = norm;
    a.records[a.record[k]] = rec;
}

struct SnAdamScalars {
    float s, wd, omb1, beta2, omb2, step_size, sqrt_bc2, eps;
};

__device__ inline void sn_adam_element(const SnAdamScalars& h, float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
    g = g * h.s;
    if (h.wd != 0.0f) g = g + h.wd * p;
    m = m + h.omb1 * (g - m);
    v = h.beta2 * v + h.omb2 * (g * g);
    const float denom = __fdiv_rn(__fsqrt_rn(v), h.sqrt_bc2) + h.eps;
    p = p - h.step_size * __fdiv_rn(m, denom);
}

__global__ __launch_bounds__(kSnAdamBlock) void sn_optim_adam_update_kernel(SnAdamArgs a) {
    const int t = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const SnAdamChunkRef r = sn_adam_locate(a.prefix, a.n_slots, a.n, c);
        const int k = r.slot;
        const SnAdamRecord rec = a.records[a.record[k]];
        if (rec.skip) continue;  // (uniform) before anything of the tensor is loaded
        SnAdamScalars h;
        h.s = rec.grad_multiplier;
        h.wd = a.weight_decay[k];
        h.omb1 = (float)(1.0 - (double)a.beta1[k]);
        h.beta2 = a.beta2[k];
        h.omb2 = (float)(1.0 - (double)a.beta2[k]);
        h.step_size = rec.step_size;
        h.sqrt_bc2 = rec.sqrt_bc2;
        h.eps = a.eps[k];
        float* p = a.param[k] + r.first;
        const float* g = a.grad[k] + r.first;
        float* m = a.exp_avg[k] + r.first;
        float* v = a.exp_avg_sq[k] + r.first;
        if ((a.vector_mask >> k) & 1u) {
            const int whole = r.count & ~3;
            for (int i = 4 * t; i < whole; i += 4 * kSnAdamBlock) {
                float4 pq = *reinterpret_cast<const float4*>(p + i);
                const float4 gq = *reinterpret_cast<const float4*>(g + i);
                float4 mq = *reinterpret_cast<const float4*>(m + i);
                float4 vq = *reinterpret_cast<const float4*>(v + i);
                sn_adam_element(h, pq.x, gq.x, mq.x, vq.x);
                sn_adam_element(h, pq.y, gq.y, mq.y, vq.y);
                sn_adam_element(h, pq.z, gq.z, mq.z, vq.z);
                sn_adam_element(h, pq.w, gq.w, mq.w, vq.w);
                *reinterpret_cast<float4*>(p + i) = pq;
                *reinterpret_cast<float4*>(m + i) = mq;
                *reinterpret_cast<float4*>(v + i) = vq;
            }
            const int i = whole + t;  // the tail, scalar: fewer than four elements
            if (i < r.count) sn_adam_element(h, p[i], g[i], m[i], v[i]);
        } else {
            for (int i = t; i < r.count; i += kSnAdamBlock) sn_adam_element(h, p[i], g[i], m[i], v[i]);
        }
    }
}
