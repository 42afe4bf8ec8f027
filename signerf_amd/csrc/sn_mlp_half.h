// sn_mlp_half.h -- the trainable MLP of sn_mlp.h in the method's mixed precision (SnMlpDesc.precision = SN_MLP_PRECISION_FP16): fp16
// operands, fp32 accumulation, fp32 master weights, on v_mfma_f32_16x16x32_f16.  Same network, same shapes of work and the same limits as
// sn_mlp.h, whose parameter block, point loads / stores and reduce kernel are used as they are; nothing in sn_mlp.h is changed.  The
// arithmetic is specified in include/signerf_hip_mlp.h and DESIGN.md §4 "Mixed-precision MLP"; tests/mlp_half_oracle.py holds it in fp64.
//
// Rounding points.  r16 = the conversion of the mode (round to nearest even, subnormals kept, overflow to inf, NaN stays NaN).
// h_0 = r16(x); z_i = sum_k r16(W_i)[o][k] h_{i-1}[k] in the MFMA's fp32 accumulator, + b_i[o] in fp32, added last; h_i = r16(relu(z_i));
// y = z_n.  Backward: the h_i are recomputed by the same code, dZ_n = r16(g), dH_{i-1} = r16(W_i)^T dZ_i in fp32,
// dZ_{i-1} = r16(dH_{i-1}) where NOT (h_{i-1} <= 0) -- the mask on the ROUNDED activation -- else 0; dx = dH_0 in fp32.  The weights are
// converted from the fp32 master copy inside the kernels, on every call: by the forward kernel as a wave loads them, by the backward kernel
// once per workgroup into LDS images (its workgroups walk many tiles and their four waves need the same fragments twice over); no packed
// copy outlives a kernel.
//
// Mapping.  Points on the MFMA's columns, 16 per wave, as in sn_mlp.h.  An activation is kept as K-blocks of 32 rows, 8 fp16 per lane and
// block: slot j of lane (i = lane & 15, h = lane >> 4) in block u is row 32 u + 16 (j >> 2) + 4 h + (j & 3) of point i -- the C/D
// registers r = j & 3 of the 16-row tiles 2 u and 2 u + 1 side by side, so two accumulator tiles ARE the next layer's B operand, and the
// A operand's lane (o, h) reads W[o][that k]: twice four consecutive floats of the nn.Linear's row.  The MFMA sums k = 8 h + j over its
// 32 slots in the hardware's order; the K-blocks are added in the order u = 0, 1 into one accumulator.  Every K-block is 32 wide: a layer
// input that is no multiple of 32 is zero-padded on both operands (the 16x16x16 form is not used).
//
// dW_i[o][k] = sum over the points of dZ_i[p][o] h_{i-1}[p][k]: the points are the K of this product, so both operands cross LDS once
// per layer as fp16 [feature][point] images (a lane writes its 2-byte elements, a fragment is one 16-byte read of 8 consecutive points).
// Wave w owns output rows 16 w .. 16 w + 15; K-block u of a tile of 64 points is its points 32 u .. 32 u + 31, slot 8 h + j = point
// 32 u + 8 h + j, and the blocks and tiles are added in index order into fp32 registers -- every product of two fp16 values is exact in
// fp32.  db_i[o] is summed in fp64 lanes.  One partial image per workgroup; sn_train_mlp_reduce_kernel adds them in fp64.  No atomics.
//
// Padding: as sn_mlp.h.  Loads return 0 outside a matrix and past N, an accumulator row past the width is SET to 0, the activations of a
// point past N are set to 0.  relu is (z <= 0 ? 0 : z) on the fp32 z: a NaN stays a NaN.
#pragma once
#include "sn_mlp.h"

#define SN_MLP_HALF_KBLOCKS 2   // 32-row K-blocks of the widest layer: SN_MLP_TILES / 2
#define SN_MLP_HALF_LD 72       // row stride, in fp16 elements, of the backward kernel's [feature][point] LDS images: rows stay 16-byte
                                // aligned, and the four row groups of a wave's 2-byte writes (4 rows = 144 dwords apart) fall on distinct banks

typedef _Float16 sn_h16x8 __attribute__((ext_vector_type(8)));

// the tiles 2 u and 2 u + 1 of an fp32 activation rounded into K-block u
SN_DEV sn_h16x8 sn_mlp_half_pack(const sn_f32x4& lo, const sn_f32x4& hi) {
    return sn_h16x8{(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3], (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2], (_Float16)hi[3]};
}

SN_DEV void sn_mlp_half_round(const sn_f32x4 (&v)[SN_MLP_TILES], sn_h16x8 (&r)[SN_MLP_HALF_KBLOCKS]) {
#pragma unroll
    for (int u = 0; u < SN_MLP_HALF_KBLOCKS; ++u) r[u] = sn_mlp_half_pack(v[2 * u], v[2 * u + 1]);
}

// The A operand of K-block u for output row `row`, lane half h: r16 of W[row][32 u + 16 (j >> 2) + 4 h + (j & 3)], j = 0..7 -- from the
// nn.Linear's fp32 matrix, converted as it arrives ...
SN_DEV sn_h16x8 sn_mlp_half_wfrag(const float* W, int din, int dout, int row, int u, int h) {
    return sn_mlp_half_pack(sn_mlp_load_row4(W, din, row, row < dout, 32 * u + 4 * h), sn_mlp_load_row4(W, din, row, row < dout, 32 * u + 16 + 4 * h));
}

// ... or from the backward kernel's [out][in] LDS image of r16(W), which holds zeros outside the matrix: two 8-byte reads
typedef _Float16 sn_h16x4 __attribute__((ext_vector_type(4)));
SN_DEV sn_h16x8 sn_mlp_half_wfrag(const _Float16* w, int, int, int row, int u, int h) {
    const sn_h16x4 lo = *reinterpret_cast<const sn_h16x4*>(w + row * SN_MLP_HALF_LD + 32 * u + 4 * h);
    const sn_h16x4 hi = *reinterpret_cast<const sn_h16x4*>(w + row * SN_MLP_HALF_LD + 32 * u + 16 + 4 * h);
    return sn_h16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// z^T = W in^T + b (relu'd for a hidden layer) for the wave's 16 points, in fp32 and in sn_mlp.h's C/D layout; `in` in K-blocks
template <typename WP>
SN_DEV void sn_mlp_half_layer(const WP* W, const float* b, int din, int dout, bool relu, const sn_h16x8 (&in)[SN_MLP_HALF_KBLOCKS],
                              sn_f32x4 (&out)[SN_MLP_TILES], int i, int h) {
#pragma unroll
    for (int to = 0; to < SN_MLP_TILES; ++to) {
        sn_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        if (16 * to < dout) {
            const int row = 16 * to + i;
#pragma unroll
            for (int u = 0; u < SN_MLP_HALF_KBLOCKS; ++u) {
                if (32 * u < din) {
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(sn_mlp_half_wfrag(W, din, dout, row, u, h), in[u], acc, 0, 0, 0);
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

__global__ __launch_bounds__(SN_MLP_BLOCK) void sn_train_mlp_half_forward_kernel(SnMlpParams p) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), i = lane & 15, h = lane >> 4;
    const int64_t n = ((int64_t)blockIdx.x * 4 + wave) * 16 + i;
    if (n - i >= p.N) return;   // (the whole wave: no point of its tile exists)
    const bool ok = n < p.N;
    sn_f32x4 c[SN_MLP_TILES];
    sn_h16x8 a[SN_MLP_HALF_KBLOCKS];
    sn_mlp_load_points(p.x, p.dims[0], n, ok, h, c);
#pragma unroll
    for (int l = 0; l < SN_MLP_LAYERS; ++l) {
        if (l < p.n_layers) {
            sn_mlp_half_round(c, a);
            sn_mlp_half_layer(p.W[l], p.b[l], p.dims[l], p.dims[l + 1], l + 1 < p.n_layers, a, c, i, h);
        }
    }
    sn_mlp_store_points(p.y, sn_mlp_out_dim(p), n, ok, h, c);
}

// the lane's 2-byte elements of an activation in K-blocks -> its column `col` of a [feature][point] image
SN_DEV void sn_mlp_half_to_lds(_Float16* img, const sn_h16x8 (&v)[SN_MLP_HALF_KBLOCKS], int dim, int col, int h) {
#pragma unroll
    for (int u = 0; u < SN_MLP_HALF_KBLOCKS; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (16 * (2 * u + (j >> 2)) < dim) img[(32 * u + 16 * (j >> 2) + 4 * h + (j & 3)) * SN_MLP_HALF_LD + col] = v[u][j];
}

__global__ __launch_bounds__(SN_MLP_BLOCK) void sn_train_mlp_half_backward_kernel(SnMlpParams p) {
    // [feature][point of the workgroup's tile] images of dZ_l and H_{l-1}: the dW product sums over the points, which sit on the lanes of
    // the tiles above, so both operands cross LDS once per layer
    __shared__ __attribute__((aligned(16))) _Float16 dz_img[16 * SN_MLP_TILES * SN_MLP_HALF_LD];
    __shared__ __attribute__((aligned(16))) _Float16 h_img[16 * SN_MLP_TILES * SN_MLP_HALF_LD];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), i = lane & 15, h = lane >> 4;
    const bool want_w = p.partials != nullptr;
    // wave w owns output rows 16 w .. 16 w + 15 of every layer's dW and db, over all the workgroup's tiles
    // (db: lane (i, h) sums dZ[.][16 w + i] over the points 32 u + 8 h + j of every tile in fp64)
    sn_f32x4 acc_w[SN_MLP_LAYERS][SN_MLP_TILES];
    double acc_b[SN_MLP_LAYERS];
#pragma unroll
    for (int l = 0; l < SN_MLP_LAYERS; ++l) {
        acc_b[l] = 0.0;
#pragma unroll
        for (int t = 0; t < SN_MLP_TILES; ++t) acc_w[l][t] = sn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    // (the widths are re-read from LDS behind a barrier in every tile, for the reason sn_train_mlp_backward_kernel gives)
    __shared__ int dims_lds[SN_MLP_LAYERS + 1];
    if (threadIdx.x <= SN_MLP_LAYERS) dims_lds[threadIdx.x] = threadIdx.x <= (unsigned)p.n_layers ? p.dims[threadIdx.x] : 0;
    // r16(W_l) as [out][in] images, zero outside the matrix, converted ONCE per workgroup: a workgroup walks ceil(tiles / P) tiles (12 at the
    // 196 608 points of a training step's main field) and its four waves need the same fragments
    __shared__ __attribute__((aligned(16))) _Float16 w_img[SN_MLP_LAYERS][16 * SN_MLP_TILES * SN_MLP_HALF_LD];
#pragma unroll
    for (int l = 0; l < SN_MLP_LAYERS; ++l) {
        if (l < p.n_layers) {
            const int din = p.dims[l], dout = p.dims[l + 1];
            for (int e = (int)threadIdx.x; e < 16 * SN_MLP_TILES * 16 * SN_MLP_TILES; e += SN_MLP_BLOCK) {
                const int o = e >> 6, k = e & 63;
                w_img[l][o * SN_MLP_HALF_LD + k] = (o < dout && k < din) ? (_Float16)p.W[l][o * din + k] : (_Float16)0.0f;
            }
        }
    }
    const int64_t tiles = (p.N + SN_MLP_WG_POINTS - 1) / SN_MLP_WG_POINTS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += p.n_partials) {   // (workgroup-uniform: the barriers below are reached by all)
        __syncthreads();   // (the first trip: the images above are complete)
        int dims[SN_MLP_LAYERS + 1];
#pragma unroll
        for (int l = 0; l <= SN_MLP_LAYERS; ++l) dims[l] = __builtin_amdgcn_readfirstlane(dims_lds[l]);
        const int64_t n = tile * SN_MLP_WG_POINTS + wave * 16 + i;
        const bool ok = n < p.N;
        sn_h16x8 hs[SN_MLP_LAYERS][SN_MLP_HALF_KBLOCKS];   // hs[l]: the input of layer l, rounded
        sn_f32x4 c[SN_MLP_TILES];
        sn_mlp_load_points(p.x, dims[0], n, ok, h, c);
        sn_mlp_half_round(c, hs[0]);
#pragma unroll
        for (int l = 0; l + 1 < SN_MLP_LAYERS; ++l) {
            if (l + 1 < p.n_layers) {
                sn_mlp_half_layer(w_img[l], p.b[l], dims[l], dims[l + 1], true, hs[l], c, i, h);
                if (!ok) {
#pragma unroll
                    for (int t = 0; t < SN_MLP_TILES; ++t) c[t] = sn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
                sn_mlp_half_round(c, hs[l + 1]);
            }
        }
        int dims_out = dims[1];
#pragma unroll
        for (int l = 2; l <= SN_MLP_LAYERS; ++l)
            if (l <= p.n_layers) dims_out = dims[l];
        sn_h16x8 dz[SN_MLP_HALF_KBLOCKS];
        sn_mlp_load_points(p.g, dims_out, n, ok, h, c);
        sn_mlp_half_round(c, dz);
#pragma unroll
        for (int l = SN_MLP_LAYERS - 1; l >= 0; --l) {
            if (l < p.n_layers) {
                const int din = dims[l], dout = dims[l + 1];
                if (want_w) {
                    sn_mlp_half_to_lds(dz_img, dz, dout, 16 * wave + i, h);
                    sn_mlp_half_to_lds(h_img, hs[l], din, 16 * wave + i, h);
                    __syncthreads();
                    if (16 * wave < dout) {
#pragma unroll
                        for (int u = 0; u < 2; ++u) {   // the tile's points 32 u .. 32 u + 31
                            const sn_h16x8 a = *reinterpret_cast<const sn_h16x8*>(dz_img + (16 * wave + i) * SN_MLP_HALF_LD + 32 * u + 8 * h);
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc_b[l] += (double)(float)a[j];
#pragma unroll
                            for (int t = 0; t < SN_MLP_TILES; ++t) {
                                if (16 * t < din) {
                                    const sn_h16x8 b = *reinterpret_cast<const sn_h16x8*>(h_img + (16 * t + i) * SN_MLP_HALF_LD + 32 * u + 8 * h);
                                    acc_w[l][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc_w[l][t], 0, 0, 0);
                                }
                            }
                        }
                    }
                    __syncthreads();
                }
                if (l > 0 || p.dx) {
                    // dH_{l-1}^T = W_l^T dZ_l^T: slot j of the A operand's lane (k, h) in K-block u reads W[32 u + 16 (j >> 2) + 4 h + (j & 3)][16 tk + k]
                    sn_f32x4 dh[SN_MLP_TILES];
#pragma unroll
                    for (int tk = 0; tk < SN_MLP_TILES; ++tk) {
                        sn_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (16 * tk < din) {
#pragma unroll
                            for (int u = 0; u < SN_MLP_HALF_KBLOCKS; ++u) {
                                if (32 * u < dout) {
                                    sn_h16x8 a;
#pragma unroll
                                    for (int j = 0; j < 8; ++j)
                                        a[j] = w_img[l][(32 * u + 16 * (j >> 2) + 4 * h + (j & 3)) * SN_MLP_HALF_LD + 16 * tk + i];
                                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, dz[u], acc, 0, 0, 0);
                                }
                            }
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                // layer l's input is a rounded relu's result for l > 0: rows past its width and padded points hold 0 there
                                if (l > 0) acc[r] = (float)hs[l][tk >> 1][4 * (tk & 1) + r] <= 0.0f ? 0.0f : acc[r];
                                else if (16 * tk + 4 * h + r >= din) acc[r] = 0.0f;
                            }
                        }
                        dh[tk] = acc;
                    }
                    if (l == 0) sn_mlp_store_points(p.dx, din, n, ok, h, dh);
                    else sn_mlp_half_round(dh, dz);
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
