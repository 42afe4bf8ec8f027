// sn_losses.h -- the back half of a training step (include/signerf_hip_losses.h): what happens AFTER the field has produced per-sample
// densities and colours.  Differentiable compositing (RaySamples.get_weights + the training-mode RGB / accumulation renderers) and
// nerfacto's two sampler losses (lossfun_distortion, lossfun_outer), each with its backward pass.  The formulas are restated from
// nerfstudio 1.0.2 [NS-RECALL] in DESIGN.md §4 "Training back half"; tests/loss_oracle.py holds them as plain torch ops.
//
// Mapping: ONE WAVE PER RAY.  Every kernel is launched with 64-thread blocks, block r works on ray r; lane l takes the samples
// l, l + 64, l + 128, ... of the [R,S] row-major rows, so every load and store of a row is coalesced.  A per-ray running sum is a wave scan
// (6 shuffle steps) with a carry from chunk to chunk, in fp64; reductions are a fixed butterfly.  No atomics anywhere: two runs on the same
// inputs give the same bits.  All loops that hold a shuffle or a barrier run a wave-uniform number of times (lanes past S carry zeros).
// Rays are independent: a non-finite value poisons its own ray only.
//
// Arithmetic: the inputs are fp32, every intermediate is fp64 (the products, exp / expm1, the scans), each output is rounded to fp32
// once.  The kernels' error against the fp64 restatement is therefore the final rounding, half an ulp per element.
#pragma once
#include "sn_device.h"

#define SN_LOSS_MAX_S 1024   // samples per ray (and envelope intervals per ray) the kernels take
#define SN_LOSS_EPS 1e-7     // nerfstudio's losses.EPS

// ---- wave primitives (64 lanes; called by every lane of the wave) -------------------------------------------------------------------------
SN_DEV double sn_loss_scan_up(double v, int lane) {   // inclusive prefix sum over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

SN_DEV double sn_loss_scan_down(double v, int lane) {   // inclusive suffix sum over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_down(v, d, 64);
        if (lane + d < 64) v += t;
    }
    return v;
}

SN_DEV double sn_loss_wave_sum(double v) {   // the same total in every lane, a fixed butterfly
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// torch.nan_to_num of the fp32 value the weight rounds to: NaN -> 0, +-inf -> +-FLT_MAX.  `finite` says whether the gradient passes.
SN_DEV double sn_loss_nan_to_num(double w, bool& finite) {
    const float wf = (float)w;
    finite = true;
    if (wf != wf) {
        finite = false;
        return 0.0;
    }
    if (wf == __builtin_inff() || wf == -__builtin_inff()) {
        finite = false;
        return wf > 0.f ? 3.4028234663852886e38 : -3.4028234663852886e38;
    }
    return w;
}

// number of a[0..n) that are <= v, for non-decreasing a: torch.searchsorted(a, v, right=True).  Bounded: at most 11 steps, result in [0, n].
template <typename T>
SN_DEV int sn_loss_count_le(const T* a, int n, T v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (a[m] <= v) lo = m + 1;
        else hi = m;
    }
    return lo;
}

// ---- compositing --------------------------------------------------------------------------------------------------------------------------
//   dd_i = delta_i * density_i,  C_i = sum_{j<i} dd_j,  T_i = exp(-C_i),  alpha_i = 1 - exp(-dd_i) = -expm1(-dd_i)
//   w_i = nan_to_num(alpha_i T_i),  acc = sum w,  rgb = sum w_i c_i + bg (1 - acc),  bg = c_{S-1} ("last_sample") or a constant
struct SnLossCompositeParams {
    const float* deltas;       // [R,S]
    const float* density;      // [R,S]
    const float* colour;       // [R,S,3] or nullptr (weights / accumulation only)
    const float* background;   // DEVICE [3] or nullptr: "last_sample"
    int S;
    // forward
    float* weights;        // [R,S] or nullptr
    float* rgb;            // [R,3] or nullptr
    float* accumulation;   // [R] or nullptr
    // backward
    const float* grad_weights;   // [R,S] or nullptr (zero)
    const float* grad_rgb;       // [R,3] or nullptr (zero)
    const float* grad_acc;       // [R] or nullptr (zero)
    float* grad_density;         // [R,S]
    float* grad_colour;          // [R,S,3] or nullptr
};

__global__ __launch_bounds__(64) void sn_loss_composite_forward_kernel(SnLossCompositeParams p) {
    const int lane = threadIdx.x, S = p.S;
    const int64_t row = (int64_t)blockIdx.x * S;
    const float* dl = p.deltas + row;
    const float* dn = p.density + row;
    const float* col = p.colour ? p.colour + row * 3 : nullptr;
    double carry = 0.0, acc = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
    for (int base = 0; base < S; base += 64) {
        const int i = base + lane;
        const bool in = i < S;
        const double dd = in ? (double)dl[i] * (double)dn[i] : 0.0;
        const double incl = sn_loss_scan_up(dd, lane) + carry;
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = carry;
        carry = __shfl(incl, 63, 64);
        bool finite;
        const double w = sn_loss_nan_to_num(-expm1(-dd) * exp(-excl), finite);
        if (in) {
            if (p.weights) p.weights[row + i] = (float)w;
            acc += w;
            if (col) {
                c0 += w * (double)col[i * 3 + 0];
                c1 += w * (double)col[i * 3 + 1];
                c2 += w * (double)col[i * 3 + 2];
            }
        }
    }
    acc = sn_loss_wave_sum(acc);
    if (p.rgb) {
        c0 = sn_loss_wave_sum(c0);
        c1 = sn_loss_wave_sum(c1);
        c2 = sn_loss_wave_sum(c2);
    }
    if (lane == 0) {
        if (p.accumulation) p.accumulation[blockIdx.x] = (float)acc;
        if (p.rgb) {
            const float* bg = p.background ? p.background : col + (int64_t)(S - 1) * 3;
            float* out = p.rgb + (int64_t)blockIdx.x * 3;
            out[0] = (float)(c0 + (double)bg[0] * (1.0 - acc));
            out[1] = (float)(c1 + (double)bg[1] * (1.0 - acc));
            out[2] = (float)(c2 + (double)bg[2] * (1.0 - acc));
        }
    }
}

// With G_i = gw_i + g_rgb . c_i + g_acc - g_rgb . bg  (the gradient that reaches w_i; 0 where nan_to_num replaced the weight):
//   d w_k / d dd_k = exp(-dd_k) T_k = T_{k+1},   d w_i / d dd_k = -w_i  (i > k)
//   grad_density_k = delta_k (G_k T_{k+1} - sum_{i>k} G_i w_i)                       -- one reverse scan per ray
//   grad_colour_i  = w_i g_rgb  (+ (1 - acc) g_rgb for i = S-1 with the "last_sample" background)
// The deltas get no gradient: nerfacto's sampler hands out detached bins.
// Pass 1 runs the forward scan of dd and leaves the carry INTO chunk c in lane c (S <= 1024: at most 16 chunks); pass 2 walks the chunks
// backwards, rebuilds each chunk's prefix from that carry and scans G_i w_i from the far end.
__global__ __launch_bounds__(64) void sn_loss_composite_backward_kernel(SnLossCompositeParams p) {
    const int lane = threadIdx.x, S = p.S;
    const int64_t row = (int64_t)blockIdx.x * S;
    const float* dl = p.deltas + row;
    const float* dn = p.density + row;
    const float* col = p.colour ? p.colour + row * 3 : nullptr;
    const float* gw = p.grad_weights ? p.grad_weights + row : nullptr;
    double carry = 0.0, chunk_carry = 0.0;
    const int chunks = (S + 63) >> 6;
    for (int c = 0; c < chunks; ++c) {
        const int i = c * 64 + lane;
        const double dd = i < S ? (double)dl[i] * (double)dn[i] : 0.0;
        if (lane == c) chunk_carry = carry;
        carry = __shfl(sn_loss_scan_up(dd, lane) + carry, 63, 64);   // the forward kernel's carry, to the bit
    }
    double g[3] = {0.0, 0.0, 0.0}, bgdot = 0.0;
    if (p.grad_rgb && col) {
        const float* bg = p.background ? p.background : col + (int64_t)(S - 1) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            g[k] = (double)p.grad_rgb[(int64_t)blockIdx.x * 3 + k];
            bgdot += g[k] * (double)bg[k];
        }
    }
    const double gbase = (p.grad_acc ? (double)p.grad_acc[blockIdx.x] : 0.0) - bgdot;
    double rcarry = 0.0;   // sum of G_i w_i over the chunks behind this one
    for (int c = chunks - 1; c >= 0; --c) {
        const int i = c * 64 + lane;
        const bool in = i < S;
        const double delta = in ? (double)dl[i] : 0.0;
        const double dd = in ? delta * (double)dn[i] : 0.0;
        const double start = __shfl(chunk_carry, c, 64);
        const double incl = sn_loss_scan_up(dd, lane) + start;
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = start;
        const double t_next = exp(-incl);   // T_{i+1}
        bool finite;
        const double w = sn_loss_nan_to_num(-expm1(-dd) * exp(-excl), finite);
        double G = gbase + (gw && in ? (double)gw[i] : 0.0);
        double ci[3] = {0.0, 0.0, 0.0};
        if (col && in) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ci[k] = (double)col[i * 3 + k];
                G += g[k] * ci[k];
            }
        }
        const bool live = in && finite;
        const double gwi = live ? G * w : 0.0;
        const double suffix = sn_loss_scan_down(gwi, lane) + rcarry;   // sum_{i' >= i}
        rcarry = __shfl(suffix, 0, 64);
        if (in) {
            const double first = live ? G * t_next : 0.0;
            p.grad_density[row + i] = (float)(delta * (first - (suffix - gwi)));
            if (p.grad_colour) {
                // T_S = exp(-sum dd) = 1 - acc: what the "last_sample" background weighs c_{S-1} with (i = S-1 => incl is the total)
                const double extra = (!p.background && i == S - 1) ? t_next : 0.0;
                float* gc = p.grad_colour + (row + i) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) gc[k] = (float)((w + extra) * g[k]);
            }
        }
    }
}

// ---- distortion loss ----------------------------------------------------------------------------------------------------------------------
//   u_i = (t_i + t_{i+1}) / 2,  inner_i = sum_j w_j |u_i - u_j|
//   L = sum_i w_i (inner_i + w_i (t_{i+1} - t_i) / 3),   dL/dw_i = 2 inner_i + (2/3) w_i (t_{i+1} - t_i);   t is a constant.
// The pairwise form: S^2 fp64 multiply-adds per ray, each lane walks j = 0..S-1 over the row staged in LDS (all lanes read the same
// address: a broadcast).  No cancellation beyond that of u_i - u_j itself, which fp64 forms exactly from the fp32 edges.
struct SnLossDistortionParams {
    const float* t;           // [R,S+1]
    const float* w;           // [R,S]
    const float* grad_loss;   // [R]  (backward)
    int S;
    float* loss;     // [R]    (forward)
    float* grad_w;   // [R,S]  (backward)
};

template <bool BACKWARD>
SN_DEV void sn_loss_distortion_ray(const SnLossDistortionParams& p, unsigned char* lds) {
    const int lane = threadIdx.x, S = p.S;
    double* u = (double*)lds;          // [S]
    float* wl = (float*)(u + S);       // [S]
    const float* t = p.t + (int64_t)blockIdx.x * (S + 1);
    const float* w = p.w + (int64_t)blockIdx.x * S;
    for (int i = lane; i < S; i += 64) {
        u[i] = ((double)t[i] + (double)t[i + 1]) * 0.5;
        wl[i] = w[i];
    }
    __syncthreads();
    const double g = BACKWARD ? (double)p.grad_loss[blockIdx.x] : 0.0;
    double total = 0.0;
    for (int i = lane; i < S; i += 64) {
        const double ui = u[i], wi = (double)wl[i];
        double inner = 0.0;
        for (int j = 0; j < S; ++j) inner += (double)wl[j] * fabs(ui - u[j]);
        const double width = (double)t[i + 1] - (double)t[i];
        if (BACKWARD) p.grad_w[(int64_t)blockIdx.x * S + i] = (float)(g * (2.0 * inner + (2.0 / 3.0) * wi * width));
        else total += wi * (inner + wi * width * (1.0 / 3.0));
    }
    if (!BACKWARD) {
        total = sn_loss_wave_sum(total);
        if (lane == 0) p.loss[blockIdx.x] = (float)total;
    }
}

extern __shared__ __attribute__((aligned(16))) unsigned char sn_loss_lds[];

__global__ __launch_bounds__(64) void sn_loss_distortion_forward_kernel(SnLossDistortionParams p) { sn_loss_distortion_ray<false>(p, sn_loss_lds); }
__global__ __launch_bounds__(64) void sn_loss_distortion_backward_kernel(SnLossDistortionParams p) { sn_loss_distortion_ray<true>(p, sn_loss_lds); }

static inline size_t sn_loss_distortion_lds(int S) { return (size_t)S * 12; }

// ---- interlevel loss ----------------------------------------------------------------------------------------------------------------------
//   lo_i = clamp(#{k < P: t_env[k] <= t_i} - 1, 0, P-1),  hi_i = clamp(#{1 <= k <= P: t_env[k] <= t_{i+1}}, 0, P-1)
//   w_outer_i = cw[hi_i + 1] - cw[lo_i],  cw[k] = sum_{j<k} w_env_j  (fp64)
//   L = (1/S) sum_i max(w_i - w_outer_i, 0)^2 / (w_i + 1e-7)
//   grad_w_env_j = sum_{i: lo_i <= j <= hi_i} c_i,   c_i = -2 max(w_i - w_outer_i, 0) / (w_i + 1e-7) g / S
// Each lane binary-searches the envelope's edges in LDS for its own samples (the one-merge form of a lane-per-ray mapping would serialise
// the wave).  Backward: t and t_env are non-decreasing, so lo and hi are too, and the rays of the difference array
//   D[j] = sum_{i: lo_i = j} c_i - sum_{i: hi_i + 1 = j} c_i
// are contiguous runs of i; its prefix sum is  grad_j = PC[#{i: lo_i <= j}] - PC[#{i: hi_i < j}]  with PC the fp64 prefix sum of c.
// Both counts are searches in the monotone lo / hi rows: no scatter, no atomics.
struct SnLossInterlevelParams {
    const float* t;           // [R,S+1]
    const float* w;           // [R,S]
    const float* t_env;       // [R,P+1]
    const float* w_env;       // [R,P]
    const float* grad_loss;   // [R]  (backward)
    int S, P;
    float* loss;         // [R]    (forward; or nullptr)
    float* w_outer;      // [R,S]  (forward; or nullptr)
    float* grad_w_env;   // [R,P]  (backward)
};

struct SnLossInterlevelLds {
    double* cw;   // [P+1]
    double* pc;   // [S+1]  (backward)
    float* te;    // [P+1]
    int* lo;      // [S]    (backward)
    int* hi;      // [S]    (backward)
};

static inline size_t sn_loss_interlevel_lds(int S, int P, bool backward) {
    return (size_t)(P + 1) * 12 + (backward ? (size_t)(S + 1) * 8 + (size_t)S * 8 : 0);
}

SN_DEV SnLossInterlevelLds sn_loss_interlevel_carve(unsigned char* lds, int S, int P) {
    SnLossInterlevelLds L;
    L.cw = (double*)lds;
    L.pc = L.cw + (P + 1);
    L.te = (float*)(L.pc + (S + 1));   // (the forward kernel's allocation ends behind te: it is carved with S = -1)
    L.lo = (int*)(L.te + (P + 1));
    L.hi = L.lo + S;
    return L;
}

// stages the envelope of this block's ray: its edges and the exclusive fp64 prefix sum of its weights; ends with a barrier
SN_DEV void sn_loss_stage_envelope(const SnLossInterlevelParams& p, const SnLossInterlevelLds& L) {
    const int lane = threadIdx.x, P = p.P;
    const float* te = p.t_env + (int64_t)blockIdx.x * (P + 1);
    const float* we = p.w_env + (int64_t)blockIdx.x * P;
    double carry = 0.0;
    for (int base = 0; base < P + 1; base += 64) {   // (P + 1 edges; the prefix sum has P + 1 entries too)
        const int k = base + lane;
        if (k <= P) L.te[k] = te[k];
        const double incl = sn_loss_scan_up(k < P ? (double)we[k] : 0.0, lane) + carry;
        carry = __shfl(incl, 63, 64);
        if (k < P) L.cw[k + 1] = incl;
    }
    if (lane == 0) L.cw[0] = 0.0;
    __syncthreads();
}

// the two interval indices of sample i and  max(w_i - w_outer_i, 0) / (w_i + eps)  (NaN is handed on, as torch.clip does)
SN_DEV void sn_loss_outer_sample(const SnLossInterlevelLds& L, int P, float t0, float t1, double wi, int& lo, int& hi, double& outer,
                                 double& excess, double& ratio) {
    lo = min(max(sn_loss_count_le(L.te, P, t0) - 1, 0), P - 1);
    hi = min(max(sn_loss_count_le(L.te + 1, P, t1), 0), P - 1);
    outer = L.cw[hi + 1] - L.cw[lo];
    const double x = wi - outer;
    excess = x < 0.0 ? 0.0 : x;
    ratio = excess / (wi + SN_LOSS_EPS);
}

__global__ __launch_bounds__(64) void sn_loss_interlevel_forward_kernel(SnLossInterlevelParams p) {
    const int lane = threadIdx.x, S = p.S, P = p.P;
    const SnLossInterlevelLds L = sn_loss_interlevel_carve(sn_loss_lds, -1, P);
    sn_loss_stage_envelope(p, L);
    const float* t = p.t + (int64_t)blockIdx.x * (S + 1);
    const float* w = p.w ? p.w + (int64_t)blockIdx.x * S : nullptr;   // (w_outer alone does not read the main weights)
    double total = 0.0;
    for (int i = lane; i < S; i += 64) {
        int lo, hi;
        double outer, excess, ratio;
        sn_loss_outer_sample(L, P, t[i], t[i + 1], w ? (double)w[i] : 0.0, lo, hi, outer, excess, ratio);
        if (p.w_outer) p.w_outer[(int64_t)blockIdx.x * S + i] = (float)outer;
        total += excess * ratio;
    }
    total = sn_loss_wave_sum(total);
    if (lane == 0 && p.loss) p.loss[blockIdx.x] = (float)(total / (double)S);
}

__global__ __launch_bounds__(64) void sn_loss_interlevel_backward_kernel(SnLossInterlevelParams p) {
    const int lane = threadIdx.x, S = p.S, P = p.P;
    const SnLossInterlevelLds L = sn_loss_interlevel_carve(sn_loss_lds, S, P);
    sn_loss_stage_envelope(p, L);
    const float* t = p.t + (int64_t)blockIdx.x * (S + 1);
    const float* w = p.w + (int64_t)blockIdx.x * S;
    const double scale = -2.0 * (double)p.grad_loss[blockIdx.x] / (double)S;
    double carry = 0.0;
    for (int base = 0; base < S; base += 64) {
        const int i = base + lane;
        double c = 0.0;
        if (i < S) {
            int lo, hi;
            double outer, excess, ratio;
            sn_loss_outer_sample(L, P, t[i], t[i + 1], (double)w[i], lo, hi, outer, excess, ratio);
            L.lo[i] = lo;
            L.hi[i] = hi;
            c = ratio * scale;
        }
        const double incl = sn_loss_scan_up(c, lane) + carry;
        carry = __shfl(incl, 63, 64);
        if (i < S) L.pc[i + 1] = incl;
    }
    if (lane == 0) L.pc[0] = 0.0;
    __syncthreads();
    float* out = p.grad_w_env + (int64_t)blockIdx.x * P;
    for (int j = lane; j < P; j += 64) {
        const int n_lo = sn_loss_count_le(L.lo, S, j);       // #{i: lo_i <= j}
        const int n_hi = sn_loss_count_le(L.hi, S, j - 1);   // #{i: hi_i < j}
        out[j] = (float)(L.pc[n_lo] - L.pc[n_hi]);
    }
}
