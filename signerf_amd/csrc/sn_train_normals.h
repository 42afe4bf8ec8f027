// sn_train_normals.h -- the analytic normals of training samples (include/signerf_hip_train_normals.h): nerfstudio's Field.get_normals
// [NS-RECALL; oracle.nerfacto.field_analytic_normals] on the caller's hash table and nn.Linear stack, in ONE kernel: the hash encoding with
// the slopes of its blend (sn_hashgrid.h's cells and nesting), the stack forwards and the one-hot gradient of output channel 0 backwards
// (sn_mlp.h's tile routines on the exact-fp32 MFMA: sn_mlp_layer forwards, the loads and the layout backwards), and the contraction of the two.  The formulas are restated in DESIGN.md §4
// "Training-mode normals"; tests/train_normals_oracle.py holds them as torch ops.
//
// Mapping: sn_mlp.h's.  A wave owns 16 points on the MFMA's columns; lane (i = lane & 15, h = lane >> 4) holds, of every 16-row tile t of
// an activation, rows 16 t + 4 h + r (r = 0..3) of point i.  The encoding is PRODUCED in that layout: the lane gathers the corner rows of
// the levels its features 16 t + 4 h .. + 3 belong to -- 4 / F levels for F <= 2, the level's four (F = 4) or half of its eight (F = 8)
// features otherwise -- and keeps, beside each feature, its three slopes d enc / d o_a.  g_enc comes back from the reverse pass in the same
// layout, so the contraction is lane-local but for the sum over the four lanes of a point (two xor shuffles: every lane of a point adds
// the same pairs and holds the same bits).  No LDS, nothing shared between points, no atomics: bit-reproducible.
//
// Arithmetic: fp32 throughout.  The features are sn_hashgrid_forward_kernel's, bit for bit (the same nesting, no contraction), so every
// ReLU mask is the one the two-launch route (sn_mlp_backward on the encoding, then sn_hashgrid_backward) sees; the slopes are the literal
// derivative of that nesting in fp32; g_a is an fmaf chain per level and lane, times the level's scale, fmaf-added over the lane's levels.
// normals = -g / max(|g|, 1e-12) with an IEEE division.  An out-of-domain point (sn_hashgrid.h "Domain") fetches nothing and gives NaN.
#pragma once
#include "sn_device.h"
#include "sn_hashgrid.h"
#include "sn_mlp.h"

struct SnTrainNormalsParams {
    const float* q;                 // [N,3]
    const float* table;             // [L*T,F]
    const float* scal;              // [L]
    float* normals;                 // [N,3]
    float* grad_q;                  // [N,3] or null
    const float* W[SN_MLP_LAYERS];  // [dims[l + 1], dims[l]]
    const float* b[SN_MLP_LAYERS];  // [dims[l + 1]]
    int64_t N;
    int32_t L, log2_T;
    int32_t n_layers;
    int32_t dims[SN_MLP_LAYERS + 1];   // dims[0] = L * F
};

// dH_in^T = W^T dZ^T for the wave's 16 points, dz / dh in the C/D layout: lane (k, h) of the A operand reads W[16 to + 4 h + s][16 tk + k].
// `hin`, the layer's input, is a relu's result unless this is the FIRST layer: its gradient passes where hin is not <= 0 (rows past its
// width and padded points hold 0 there); the first layer's rows past the input width are set to 0.
// This is the reverse step of sn_train_mlp_backward_kernel (sn_mlp.h), which keeps its own inline copy, so sn_mlp.h is untouched: called
// from there the routine changed that kernel's code in both forms tried -- with FIRST as a function argument 12 more AGPRs and one wave
// per SIMD instead of two, with FIRST as a template argument the same registers but other compares and another instruction order, which
// an A/B of the backward pass could not tell from the parent's (DESIGN.md §4 "Training-mode normals", "The reverse step").
template <bool FIRST>
SN_DEV void sn_mlp_layer_grad_in(const float* W, int din, int dout, const sn_f32x4 (&dz)[SN_MLP_TILES],
                                 const sn_f32x4 (&hin)[SN_MLP_TILES], sn_f32x4 (&dh)[SN_MLP_TILES], int i, int h) {
#pragma unroll
    for (int tk = 0; tk < SN_MLP_TILES; ++tk) {
        sn_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        if (16 * tk < din) {
#pragma unroll
            for (int to = 0; to < SN_MLP_TILES; ++to) {
                if (16 * to < dout) {
                    const sn_f32x4 a = sn_mlp_load_col4(W, dout, din, 16 * to + 4 * h, 16 * tk + i);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], dz[to][s], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (!FIRST) acc[r] = hin[tk][r] <= 0.0f ? 0.0f : acc[r];
                else if (16 * tk + 4 * h + r >= din) acc[r] = 0.0f;
            }
        }
        dh[tk] = acc;
    }
}

template <int F>
__global__ __launch_bounds__(SN_MLP_BLOCK) void sn_train_normals_analytic_kernel(SnTrainNormalsParams p) {
    constexpr int NF = F >= 4 ? 4 : F;   // features of ONE level in a lane's run of four
    constexpr int LV = 4 / NF;           // levels in that run
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), i = lane & 15, h = lane >> 4;
    const int64_t n = ((int64_t)blockIdx.x * 4 + wave) * 16 + i;
    if (n - i >= p.N) return;   // (the whole wave: no point of its tile exists)
    const bool ok = n < p.N;
    float q[3] = {0.0f, 0.0f, 0.0f};
    bool dom = false;
    if (ok) {
        q[0] = p.q[n * 3];
        q[1] = p.q[n * 3 + 1];
        q[2] = p.q[n * 3 + 2];
        dom = sn_hg_in_domain(q, p.scal, p.L);
    }
    const int din = p.dims[0];
    sn_f32x4 hs[SN_MLP_LAYERS][SN_MLP_TILES];   // hs[l]: the input of layer l; hs[0] is the encoding
    sn_f32x4 slope[3][SN_MLP_TILES];            // d enc / d o_a of the same features
#pragma unroll
    for (int t = 0; t < SN_MLP_TILES; ++t) {
        hs[0][t] = slope[0][t] = slope[1][t] = slope[2][t] = sn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (16 * t < din) {
#pragma unroll
            for (int j = 0; j < LV; ++j) {
                const int k0 = 16 * t + 4 * h + j * NF, l = k0 / F, f0 = k0 % F;
                if (dom && l < p.L) {
                    uint32_t row[8];
                    float o[3];
                    sn_hg_cell(q, p.scal[l], l, p.log2_T, row, o);
                    SnHgRow<NF> c[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) c[k] = sn_hg_load<NF>(p.table + row[k] * (uint32_t)F + f0);
                    {
#pragma clang fp contract(off)
                        const float ox = o[0], oy = o[1], oz = o[2], rx = 1.0f - ox, ry = 1.0f - oy, rz = 1.0f - oz;
#pragma unroll
                        for (int f = 0; f < NF; ++f) {
                            const float f03 = c[0].v[f] * ox + c[3].v[f] * rx;
                            const float f12 = c[1].v[f] * ox + c[2].v[f] * rx;
                            const float f56 = c[5].v[f] * ox + c[6].v[f] * rx;
                            const float f47 = c[4].v[f] * ox + c[7].v[f] * rx;
                            const float f0312 = f03 * oy + f12 * ry;
                            const float f4756 = f47 * oy + f56 * ry;
                            hs[0][t][j * NF + f] = f0312 * oz + f4756 * rz;
                            slope[0][t][j * NF + f] = ((c[0].v[f] - c[3].v[f]) * oy + (c[1].v[f] - c[2].v[f]) * ry) * oz +
                                                      ((c[4].v[f] - c[7].v[f]) * oy + (c[5].v[f] - c[6].v[f]) * ry) * rz;
                            slope[1][t][j * NF + f] = (f03 - f12) * oz + (f47 - f56) * rz;
                            slope[2][t][j * NF + f] = f0312 - f4756;
                        }
                    }
                }
            }
        }
    }
    // the hidden activations (the last layer's output is not needed: only its weights' row 0 is)
#pragma unroll
    for (int l = 0; l + 1 < SN_MLP_LAYERS; ++l)
        if (l + 1 < p.n_layers) sn_mlp_layer(p.W[l], p.b[l], p.dims[l], p.dims[l + 1], true, hs[l], hs[l + 1], i, h);
    // dZ_n = the one-hot of output channel 0 (row 0 of tile 0: lane h = 0, register 0), then back to the encoding
    sn_f32x4 dz[SN_MLP_TILES];
#pragma unroll
    for (int t = 0; t < SN_MLP_TILES; ++t) dz[t] = sn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    dz[0][0] = h == 0 ? 1.0f : 0.0f;
#pragma unroll
    for (int l = SN_MLP_LAYERS - 1; l >= 0; --l) {
        if (l < p.n_layers) {
            sn_f32x4 dh[SN_MLP_TILES];
            if (l == 0) sn_mlp_layer_grad_in<true>(p.W[l], p.dims[l], p.dims[l + 1], dz, hs[l], dh, i, h);
            else sn_mlp_layer_grad_in<false>(p.W[l], p.dims[l], p.dims[l + 1], dz, hs[l], dh, i, h);
#pragma unroll
            for (int t = 0; t < SN_MLP_TILES; ++t) dz[t] = dh[t];
        }
    }
    // g_a = sum_l s_l sum_f g_enc[l, f] slope[l, f, a]: this lane's levels, then the four lanes of the point
    float g[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < SN_MLP_TILES; ++t) {
        if (16 * t < din) {
#pragma unroll
            for (int j = 0; j < LV; ++j) {
                const int l = (16 * t + 4 * h + j * NF) / F;
                if (l < p.L) {
                    const float s = p.scal[l];
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        float in = 0.0f;
#pragma unroll
                        for (int f = 0; f < NF; ++f) in = __builtin_fmaf(dz[t][j * NF + f], slope[a][t][j * NF + f], in);
                        g[a] = __builtin_fmaf(s, in, g[a]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g[a] += __shfl_xor(g[a], 16, 64);
        g[a] += __shfl_xor(g[a], 32, 64);
    }
    if (!ok || h != 0) return;
    float* out = p.normals + n * 3;
    float* raw = p.grad_q ? p.grad_q + n * 3 : nullptr;
    if (!dom) {
        out[0] = out[1] = out[2] = __builtin_nanf("");
        if (raw) raw[0] = raw[1] = raw[2] = __builtin_nanf("");
        return;
    }
    const float norm = __builtin_sqrtf(__builtin_fmaf(g[2], g[2], __builtin_fmaf(g[1], g[1], g[0] * g[0])));
    const float den = norm < 1e-12f ? 1e-12f : norm;   // F.normalize: v / max(|v|, eps)  (a NaN norm stays)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[a] = -g[a] / den;
        if (raw) raw[a] = g[a];
    }
}
