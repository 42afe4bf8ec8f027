// sn_mlp.h -- the trainable MLP (include/signerf_hip_mlp.h): nerfstudio's torch MLP [SURVEY.md A8] -- h_0 = x, z_i = h_{i-1} W_i^T + b_i,
// h_i = relu(z_i), no activation after the last layer -- on the [out, in] row-major weights an nn.Linear holds, forward and backward, on the
// exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).  Nothing is packed and nothing is kept between the passes: the backward kernel recomputes the
// hidden activations of its tile.  The formulas are restated in DESIGN.md §4 "Trainable MLP"; tests/mlp_oracle.py holds them as torch ops.
//
// Mapping.  Points sit on the MFMA's columns: a wave owns 16 points and computes H_out^T = W H_in^T, 16 output rows per tile.  Lane
// (i = lane & 15, h = lane >> 4) holds, of every 16-row tile t of an activation, rows 16 t + 4 h + r (r = 0..3) of point i -- the MFMA's
// C/D layout -- and that tile is the next layer's B operand as it stands: in step s of tile t lane (i, h) supplies register s, so the step
// sums k = 16 t + 4 h + s over h = 0..3, and the A operand's lane (o, h) reads W[o][16 t + 4 h + s] (for s = 0..3 four consecutive floats
// of the nn.Linear's row).  x and g are loaded in the same permuted order.  No LDS on the forward path.
//
// Arithmetic.  An fp32 MFMA is a k-ordered fmaf chain, so z_i[o] = ((chain from 0 over t = 0.., s = 0..3, h = 0..3 of
// W[o][16 t + 4 h + s] h[16 t + 4 h + s]) + b[o]): the bias is added last.  dH_{i-1}[k] is the same chain over o.  dW_i[o][k] is, per
// workgroup, ONE chain from 0 over the workgroup's points in the order (tile; s = 0..15; h = 0..3 -> point 64 tile + 4 s + h); db_i[o] is a
// plain sum, formed per workgroup in fp64 and rounded once; a second kernel adds the workgroups' partial images in index order in fp64 and
// rounds once.  No float atomics anywhere, so
// all five outputs are bit-reproducible, and the number of partials depends on N alone.
//
// Padding.  Rows past a layer's width, columns past its input and points past N are exact zeros on BOTH operands: the loads return 0 outside
// the matrix, and an accumulator row past the width is SET to 0 (0 x inf from a zero weight row would otherwise hand a NaN to the next
// layer); the activations of a point past N are set to 0 in the backward kernel, so relu(b) of a padded point never meets dW.
// NaN.  relu is (z <= 0 ? 0 : z): a NaN stays a NaN, as in torch (v_max_f32 alone would return 0).  The backward mask is torch's
// threshold_backward on the relu's result, (h <= 0 ? 0 : dH): a NaN activation lets its gradient pass.
#pragma once
#include "sn_device.h"

#define SN_MLP_LAYERS 4          // = SN_MLP_MAX_LAYERS of the header
#define SN_MLP_TILES 4           // 16-row tiles of the widest layer: SN_MLP_MAX_DIM / 16
#define SN_MLP_BLOCK 256
#define SN_MLP_WG_POINTS 64      // 4 waves of 16 points (signerf_amd/mlp.py restates this and SN_MLP_MAX_PARTIALS as WG_POINTS, MAX_PARTIALS:
                                 // tests/test_mlp_host.py holds its workspace size against sn_mlp_backward_workspace_bytes)
#define SN_MLP_LD 68             // row stride of the backward kernel's [point][feature] LDS images: rows stay 16-byte aligned
#define SN_MLP_MAX_PARTIALS 256  // partial dW / db images of one backward call: min(ceil(N / 64), this)

typedef float sn_f32x4 __attribute__((ext_vector_type(4)));

struct SnMlpParams {
    const float* x;                 // [N, dims[0]]
    const float* g;                 // [N, dims[n]]
    float* y;                       // [N, dims[n]]
    float* dx;                      // [N, dims[0]] or null
    float* partials;                // [n_partials, image] or null (no weight gradients)
    const float* W[SN_MLP_LAYERS];  // [dims[l + 1], dims[l]]
    const float* b[SN_MLP_LAYERS];  // [dims[l + 1]]
    float* dW[SN_MLP_LAYERS];
    float* db[SN_MLP_LAYERS];
    int64_t N;
    int32_t n_layers;
    int32_t dims[SN_MLP_LAYERS + 1];
    int32_t n_partials;
    int32_t image;                  // floats of one partial image: sum over the layers of out * in + out
};

// elements [row][col0 + s], s = 0..3, of a row-major matrix with `cols` columns; 0 where !row_ok or past the last column
SN_DEV sn_f32x4 sn_mlp_load_row4(const float* m, int cols, int64_t row, bool row_ok, int col0) {
    sn_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row_ok) {
        const float* p = m + row * cols + col0;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (col0 + s < cols) v[s] = p[s];
    }
    return v;
}

// elements [row0 + s][col], s = 0..3, of a row-major [rows, cols] matrix; 0 outside it
SN_DEV sn_f32x4 sn_mlp_load_col4(const float* m, int rows, int cols, int row0, int col) {
    sn_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (col < cols) {
        const float* p = m + row0 * cols + col;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (row0 + s < rows) v[s] = p[s * cols];
    }
    return v;
}

// out^T = act(W in^T + b) for the wave's 16 points; in / out in the C/D layout described above
SN_DEV void sn_mlp_layer(const float* W, const float* b, int din, int dout, bool relu, const sn_f32x4 (&in)[SN_MLP_TILES],
                         sn_f32x4 (&out)[SN_MLP_TILES], int i, int h) {
#pragma unroll
    for (int to = 0; to < SN_MLP_TILES; ++to) {
        sn_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        if (16 * to < dout) {
            const int row = 16 * to + i;
#pragma unroll
            for (int tk = 0; tk < SN_MLP_TILES; ++tk) {
                if (16 * tk < din) {
                    const sn_f32x4 a = sn_mlp_load_row4(W, din, row, row < dout, 16 * tk + 4 * h);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], in[tk][s], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 16 * to + 4 * h + r;
                float z = 0.0f;
                if (o < dout) {
                    z = acc[r] + b[o];
                    if (relu) z = z <= 0.0f ? 0.0f : z;   // (a NaN fails the comparison and stays)
                }
                acc[r] = z;
            }
        }
        out[to] = acc;
    }
}

// dims[n_layers] without a dynamic index into the kernel's arguments
SN_DEV int sn_mlp_out_dim(const SnMlpParams& p) {
    int d = p.dims[1];
#pragma unroll
    for (int l = 2; l <= SN_MLP_LAYERS; ++l)
        if (l <= p.n_layers) d = p.dims[l];
    return d;
}

SN_DEV void sn_mlp_load_points(const float* m, int cols, int64_t n, bool ok, int h, sn_f32x4 (&v)[SN_MLP_TILES]) {
#pragma unroll
    for (int t = 0; t < SN_MLP_TILES; ++t) {
        v[t] = sn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (16 * t < cols) v[t] = sn_mlp_load_row4(m, cols, n, ok, 16 * t + 4 * h);
    }
}

SN_DEV void sn_mlp_store_points(float* m, int cols, int64_t n, bool ok, int h, const sn_f32x4 (&v)[SN_MLP_TILES]) {
    if (!ok) return;
    float* p = m + n * cols;
#pragma unroll
    for (int t = 0; t < SN_MLP_TILES; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * t + 4 * h + r < cols) p[16 * t + 4 * h + r] = v[t][r];
}

__global__ __launch_bounds__(SN_MLP_BLOCK) void sn_train_mlp_forward_kernel(SnMlpParams p) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), i = lane & 15, h = lane >> 4;
    const int64_t n = ((int64_t)blockIdx.x * 4 + wave) * 16 + i;
    if (n - i >= p.N) return;   // (the whole wave: no point of its tile exists)
    const bool ok = n < p.N;
    sn_f32x4 a[SN_MLP_TILES], c[SN_MLP_TILES];
    sn_mlp_load_points(p.x, p.dims[0], n, ok, h, a);
#pragma unroll
    for (int l = 0; l < SN_MLP_LAYERS; ++l) {
        if (l < p.n_layers) {
            sn_mlp_layer(p.W[l], p.b[l], p.dims[l], p.dims[l + 1], l + 1 < p.n_layers, a, c, i, h);
#pragma unroll
            for (int t = 0; t < SN_MLP_TILES; ++t) a[t] = c[t];
        }
    }
    sn_mlp_store_points(p.y, sn_mlp_out_dim(p), n, ok, h, a);
}

__global__ __launch_bounds__(SN_MLP_BLOCK) void sn_train_mlp_backward_kernel(SnMlpParams p) {
    // [point of the workgroup's tile][feature] images of dZ_l and H_{l-1}: the dW product sums over the points, which sit on the lanes of
    // the tiles above, so both operands cross LDS once per layer
    __shared__ __attribute__((aligned(16))) float dz_img[SN_MLP_WG_POINTS * SN_MLP_LD];
    __shared__ __attribute__((aligned(16))) float h_img[SN_MLP_WG_POINTS * SN_MLP_LD];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), i = lane & 15, h = lane >> 4;
    const bool want_w = p.partials != nullptr;
    // wave w owns output rows 16 w .. 16 w + 15 of every layer's dW and db, over all the workgroup's tiles
    // (db: lane (i, h) sums dZ[.][16 w + i] over the points 4 s + h of every tile in fp64 -- a plain sum of up to N terms, which an
    // fp32 chain would hold to no better than a few ulp of the result)
    sn_f32x4 acc_w[SN_MLP_LAYERS][SN_MLP_TILES];
    double acc_b[SN_MLP_LAYERS];
#pragma unroll
    for (int l = 0; l < SN_MLP_LAYERS; ++l) {
        acc_b[l] = 0.0;
#pragma unroll
        for (int t = 0; t < SN_MLP_TILES; ++t) acc_w[l][t] = sn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    // The widths are re-read from LDS behind a barrier in every tile: as kernel arguments they are loop-invariant, and the compiler then
    // hoists the several hundred lane masks of the bounds checks below out of the tile loop and spills them.
    __shared__ int dims_lds[SN_MLP_LAYERS + 1];
    if (threadIdx.x <= SN_MLP_LAYERS) dims_lds[threadIdx.x] = threadIdx.x <= (unsigned)p.n_layers ? p.dims[threadIdx.x] : 0;
    const int64_t tiles = (p.N + SN_MLP_WG_POINTS - 1) / SN_MLP_WG_POINTS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += p.n_partials) {   // (workgroup-uniform: the barriers below are reached by all)
        __syncthreads();
        int dims[SN_MLP_LAYERS + 1];
#pragma unroll
        for (int l = 0; l <= SN_MLP_LAYERS; ++l) dims[l] = __builtin_amdgcn_readfirstlane(dims_lds[l]);
        const int64_t n = tile * SN_MLP_WG_POINTS + wave * 16 + i;
        const bool ok = n < p.N;
        sn_f32x4 hs[SN_MLP_LAYERS][SN_MLP_TILES];   // hs[l]: the input of layer l
        sn_mlp_load_points(p.x, dims[0], n, ok, h, hs[0]);
#pragma unroll
        for (int l = 0; l + 1 < SN_MLP_LAYERS; ++l) {
            if (l + 1 < p.n_layers) {
                sn_mlp_layer(p.W[l], p.b[l], dims[l], dims[l + 1], true, hs[l], hs[l + 1], i, h);
                if (!ok) {
#pragma unroll
                    for (int t = 0; t < SN_MLP_TILES; ++t) hs[l + 1][t] = sn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
            }
        }
        int dims_out = dims[1];
#pragma unroll
        for (int l = 2; l <= SN_MLP_LAYERS; ++l)
            if (l <= p.n_layers) dims_out = dims[l];
        sn_f32x4 dz[SN_MLP_TILES];
        sn_mlp_load_points(p.g, dims_out, n, ok, h, dz);
#pragma unroll
        for (int l = SN_MLP_LAYERS - 1; l >= 0; --l) {
            if (l < p.n_layers) {
                const int din = dims[l], dout = dims[l + 1];
                if (want_w) {
                    const int row = (16 * wave + i) * SN_MLP_LD + 4 * h;
#pragma unroll
                    for (int t = 0; t < SN_MLP_TILES; ++t) {
                        if (16 * t < dout) *reinterpret_cast<sn_f32x4*>(dz_img + row + 16 * t) = dz[t];
                        if (16 * t < din) *reinterpret_cast<sn_f32x4*>(h_img + row + 16 * t) = hs[l][t];
                    }
                    __syncthreads();
                    if (16 * wave < dout) {
                        float a[16];
#pragma unroll
                        for (int s = 0; s < 16; ++s) a[s] = dz_img[(4 * s + h) * SN_MLP_LD + 16 * wave + i];
#pragma unroll
                        for (int s = 0; s < 16; ++s) acc_b[l] += (double)a[s];
#pragma unroll
                        for (int t = 0; t < SN_MLP_TILES; ++t) {
                            if (16 * t < din) {
#pragma unroll
                                for (int s = 0; s < 16; ++s)
                                    acc_w[l][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], h_img[(4 * s + h) * SN_MLP_LD + 16 * t + i],
                                                                                       acc_w[l][t], 0, 0, 0);
                            }
                        }
                    }
                    __syncthreads();
                }
                if (l > 0 || p.dx) {
                    // dH_{l-1}^T = W_l^T dZ_l^T: lane (k, h) of the A operand reads W[16 to + 4 h + s][16 tk + k]
                    sn_f32x4 dh[SN_MLP_TILES];
#pragma unroll
                    for (int tk = 0; tk < SN_MLP_TILES; ++tk) {
                        sn_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (16 * tk < din) {
#pragma unroll
                            for (int to = 0; to < SN_MLP_TILES; ++to) {
                                if (16 * to < dout) {
                                    const sn_f32x4 a = sn_mlp_load_col4(p.W[l], dout, din, 16 * to + 4 * h, 16 * tk + i);
#pragma unroll
                                    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], dz[to][s], acc, 0, 0, 0);
                                }
                            }
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                // layer l's input is a relu's result for l > 0: rows past its width and padded points hold 0 there
                                if (l > 0) acc[r] = hs[l][tk][r] <= 0.0f ? 0.0f : acc[r];
                                else if (16 * tk + 4 * h + r >= din) acc[r] = 0.0f;
                            }
                        }
                        dh[tk] = acc;
                    }
                    if (l == 0) sn_mlp_store_points(p.dx, din, n, ok, h, dh);
#pragma unroll
                    for (int t = 0; t < SN_MLP_TILES; ++t) dz[t] = dh[t];
                }
            }
        }
    }
    if (!want_w) return;
    float* img = p.partials + (int64_t)blockIdx.x * p.image;
    int off = 0;
#pragma unroll
    for (int l = 0; l < SN_MLP_LAYERS; ++l) {
        if (l < p.n_layers) {
            const int din = p.dims[l], dout = p.dims[l + 1];
            // db: the four lanes (i, h = 0..3) of output row 16 w + i add up, in the same order on every lane
            double sb = acc_b[l];
            sb += __shfl_xor(sb, 16, 64);
            sb += __shfl_xor(sb, 32, 64);
            if (h == 0 && 16 * wave + i < dout) img[off + dout * din + 16 * wave + i] = (float)sb;
            // C/D layout of the dW tiles: column (lane & 15) is the input feature, row 4 h + r the output row of the wave's 16
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 16 * wave + 4 * h + r;
                if (o < dout) {
#pragma unroll
                    for (int t = 0; t < SN_MLP_TILES; ++t)
                        if (16 * t + i < din) img[off + o * din + 16 * t + i] = acc_w[l][t][r];
                }
            }
            off += dout * din + dout;
        }
    }
}

// dW_l / db_l = the partial images added in index order, one thread per element
__global__ __launch_bounds__(SN_MLP_BLOCK) void sn_train_mlp_reduce_kernel(SnMlpParams p) {
    const int e = (int)(blockIdx.x * SN_MLP_BLOCK + threadIdx.x);
    if (e >= p.image) return;
    double sum64 = 0.0;   // (up to 256 terms: fp64 keeps the one rounding at the end)
    for (int k = 0; k < p.n_partials; ++k) sum64 += (double)p.partials[(int64_t)k * p.image + e];
    const float sum = (float)sum64;
    int off = 0;
#pragma unroll
    for (int l = 0; l < SN_MLP_LAYERS; ++l) {
        if (l < p.n_layers) {
            const int nw = p.dims[l + 1] * p.dims[l], nb = p.dims[l + 1];
            if (e >= off && e < off + nw) p.dW[l][e - off] = sum;
            if (e >= off + nw && e < off + nw + nb) p.db[l][e - off - nw] = sum;
            off += nw + nb;
        }
    }
}
