// sn_wide_kernels.h -- the render and stage kernels of a WIDE main field: hidden_dim = hidden_dim_color = 128 (nerfstudio's
// `nerfacto-big`), exact fp32 MFMA only (DESIGN.md §4 "Wide fields").
//
// The march is sn_render_main_kernel's (sn_main.h): lane = ray, wave = 8x8 pixel tile, workgroup = 2x2 tiles, one sample per lane per
// step, the strict position arithmetic (sn_sample_q), the uploaded hash table with the run-time dense / hashed decision per level, the
// same SnComposite / sn_main_epilogue / NaN restoration.  What differs is the field evaluation:
//   32 -> 128 (ReLU) -> 16;  (16 layer-2 rows | 16 SH) -> 128 (ReLU) -> 128 (ReLU) -> 3 + sigmoid
// on v_mfma_f32_32x32x2_f32 with the weights as the A operand out of an LDS image (SnWideImg) and the activations as the B operand, so
// that -- as in sn_main_field_f32 -- a layer's accumulators are the next layer's operands without leaving their registers.
//
// Registers: a 128-wide layer is four 32-row tiles.  Both 32-sample tiles of the wave at once would need 2 x (64 operand + 64
// accumulator) registers for colour layer 2 alone, so the wave's two sample tiles are evaluated ONE AFTER THE OTHER (sn_wide_field_tile);
// only the first layer's operands, the SH operands and the 16 layer-2 rows + 3 colour partial sums of tile 0 live across the two.
// Colour layer 2 runs in two passes of two row tiles whose outputs are consumed by the VALU colour layer 3 at once.
//
// Occupancy: the image is 117 904 B of LDS (+ up to 4 112 B of bins), so ONE workgroup of 4 waves per CU = 1 wave per SIMD; the kernels
// are compiled for exactly that (__launch_bounds__(256, 1): up to 512 registers, no scratch).  One wave per SIMD leaves the hash
// gathers' latency exposed.  Measured (tools/wide_bench.py, profiles/wide_bench.json): 20.1 ms per 800x800x64 frame, 2.77 x the
// default-width exact-fp32 kernel, against 2.8 x from the MFMA count; 896 fp32 MFMAs x 64 cycles per wave-step are 35.8 M cycles per SIMD
// for that frame, 18-20 ms at the sustained clock.  No counters were collected for these kernels.
#pragma once
#include "sn_device.h"
#include "sn_layout.h"
#include "sn_main.h"
#include "sn_stage.h"

// acc[rt] <- bias + W . op for ONE 32-sample tile (exact fp32 MFMA); RT independent accumulator chains.  BIAS_LAST: the bias behind
// the products instead of in front of them (sn_mlp_layer_f32: the density layer, whose 64 accumulation steps otherwise round at the bias's size)
template <int RT, int KS, bool BIAS_LAST = false>
SN_DEV void sn_wide_layer(const float* __restrict__ wimg, int rt_stride_floats, const float* __restrict__ bimg, const float* op, f32x16* acc, int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        acc[rt] = f32x16{};
        if (!BIAS_LAST) {
            const f32x4* b = (const f32x4*)(bimg + (rt * 2 + h) * 16);
            const f32x4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
            acc[rt] = f32x16{b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
        }
    }
#pragma unroll
    for (int t4 = 0; t4 < KS / 4; ++t4) {
        f32x4 a[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) a[rt] = *(const f32x4*)(wimg + rt * rt_stride_floats + (t4 * 64 + lane) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[rt][e], op[4 * t4 + e], acc[rt], 0, 0, 0);
    }
    if (BIAS_LAST) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const float* b = bimg + (rt * 2 + h) * 16;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rt][r] += b[r];
        }
    }
}

// One 32-sample tile through the whole field.  op_in[16]: the tile's hash features in B-operand order (k-step t, lane half h <-> feature
// 2t + h of sample lane & 31); sh8[8]: its SH operands (SnShOps).  g: the 32 padded layer-2 rows in accumulator order (row 0 = h0, rows
// 1..15 = geometry features, row 20 = h0 again); part[n]: this lane's partial sum of colour layer 3, channel n, over the hidden units its
// lane half holds (the other half's partial sum sits in lane ^ 32).
SN_DEV void sn_wide_field_tile(const float* __restrict__ lds, const float* op_in, const float* sh8, int lane, f32x16& g, float part[3]) {
    const int h = lane >> 5;
    float op[64];
    // ---- layer 1: 32 -> 128, ReLU ----
    {
        f32x16 a[4];
        sn_wide_layer<4, 16>(lds + SnWideImg::W1, 1024, lds + SnWideImg::B1, op_in, a, lane);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) op[rt * 16 + r] = sn_relu(a[rt][r]);
    }
    // (scheduler fences between layers: otherwise the LDS weight reads of the whole MLP are hoisted to the top)
    __builtin_amdgcn_sched_barrier(0);
    // ---- layer 2: 128 -> 16 (32 padded rows) ----
    {
        f32x16 a[1];
        sn_wide_layer<1, 64, true>(lds + SnWideImg::W2, 0, lds + SnWideImg::B2, op, a, lane);
        g = a[0];
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- colour layer 1: (layer-2 registers 0..7 = rows rho(t) + 4h | SH16) -> 128, ReLU ----
    {
        float opc[16];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            opc[t] = g[t];
            opc[8 + t] = sh8[t];
        }
        f32x16 a[4];
        sn_wide_layer<4, 16>(lds + SnWideImg::WC1, 1024, lds + SnWideImg::BC1, opc, a, lane);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) op[rt * 16 + r] = sn_relu(a[rt][r]);
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- colour layer 2: 128 -> 128, ReLU, two row tiles at a time; colour layer 3 (128 -> 3) on the VALU behind each pass ----
    part[0] = part[1] = part[2] = 0.0f;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        f32x16 c[2];
        sn_wide_layer<2, 64>(lds + SnWideImg::WC2 + pass * 2 * 4096, 4096, lds + SnWideImg::BC2 + pass * 64, op, c, lane);
        __builtin_amdgcn_sched_barrier(0);
        float x[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) x[j] = sn_relu(c[j >> 4][j & 15]);
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            const f32x4* w = (const f32x4*)(lds + SnWideImg::W3 + (n * 2 + h) * 64 + pass * 32);
#pragma unroll
            for (int j4 = 0; j4 < 8; ++j4) {
                const f32x4 wv = w[j4];
#pragma unroll
                for (int e = 0; e < 4; ++e) part[n] = fmaf(wv[e], x[4 * j4 + e], part[n]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Full wide-field evaluation of the wave's 64 samples: feat[32] = this lane's own hash features.  Returns the lane's own pre-activation
// density h0 and post-sigmoid rgb; GEO: geo16[k] = layer-2 output k of the lane's own sample (sn_main_field_f32).
template <bool GEO = false>
SN_DEV void sn_wide_field_f32(const float* __restrict__ lds, const float* feat, const SnShOps& sh, int lane, float& h0, float rgb[3],
                              float* geo16 = nullptr) {
    const bool upper = lane >= 32;
    float op0[16], op1[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        float a = feat[2 * t], b = feat[2 * t + 1];
        sn_swap_halves(a, b);
        op0[t] = a;
        op1[t] = b;
    }
    f32x16 g0, g1;
    float p0[3], p1[3];
    sn_wide_field_tile(lds, op0, sh.t0, lane, g0, p0);
    __builtin_amdgcn_sched_barrier(0);
    sn_wide_field_tile(lds, op1, sh.t1, lane, g1, p1);
    __builtin_amdgcn_sched_barrier(0);
    h0 = upper ? g1[8] : g0[0];  // lower lanes: row 0 of tile 0; upper lanes: row 20 (= row 0 again) of tile 1
    if (GEO) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float a = g0[r], b = g1[r];
            sn_swap_halves(a, b);  // every lane: a = row rho(r), b = row rho(r) + 4 of its OWN sample
            geo16[(r & 3) + 8 * (r >> 2)] = a;
            geo16[(r & 3) + 8 * (r >> 2) + 4] = b;
        }
    }
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        float a = p0[n], b = p1[n];
        sn_swap_halves(a, b);  // lower: own tile-0 partial + the upper partner's tile-0 partial; upper: the same of tile 1
        const float x = a + b + lds[SnWideImg::B3 + n];
        rgb[n] = __builtin_amdgcn_rcpf(1.0f + sn_exp<true>(-x));
    }
}

// cooperative copy of the weight image into LDS (the caller synchronises)
SN_DEV void sn_wide_load_image(float* lds, const float* __restrict__ wimg, int tid) {
    for (int i = tid * 4; i < SnWideImg::TOTAL; i += 256 * 4) *(f32x4*)(lds + i) = *(const f32x4*)(wimg + i);
}

// (Names: tests/test_launch_variants_host.py numbers the kernels a render call launches by their place in the sorted list of ALL mangled
// kernel names of the library, so a new kernel must sort behind every kernel of the default path -- _Z23sn_clip_expected_kernel is the
// last of them.  Both names here are longer than 23 characters for that reason.)
// K1, wide.  MODE: 0 uniform-in-s bins, 1 the proposal kernel's bins; GRID: 0 nerfstudio torch-path hash grid, 1 tiny-cuda-nn grid.
// Parameters: SnMainParams, of which the wide kernel reads the ray, bin, table, image, output, sampler and background fields; there is no
// split-depth tail, no de-hashed copy, no instrumentation.  Early termination is sn_render_main_kernel's (bit-identical outputs).
template <int MODE, int GRID>
__global__ __launch_bounds__(256, 1) void sn_wide_field_main_kernel(SnMainParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int su = p.spacing_uniform;
    const SnPosMap* pm = &p.pm;
    sn_wide_load_image(lds, p.wimg, tid);
    float* etab = lds + SnWideImg::TOTAL;
    const bool shared_bins = MODE == 0 && p.nears == nullptr;
    if (shared_bins) {
        const float sn = sn_spacing(p.near_plane, su), sf = sn_spacing(p.far_plane, su);
        for (int i = tid; i <= p.n_samples; i += 256) etab[i] = sn_euclid(p.sbins ? p.sbins[i] : (float)i / (float)p.n_samples, sn, sf, su);
    }
    __syncthreads();

    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int bx, by;
    sn_main_wg_coords(p, (int)blockIdx.x, bx, by);
    const int tx = bx * 2 + (wave & 1);
    const int ty = by * 2 + (wave >> 1);
    if (tx >= p.tiles_x || ty >= p.tiles_y) return;  // wave-uniform
    const int tw = 1 << p.tile_w_log2;
    const int px = (tx << p.tile_w_log2) + (lane & (tw - 1));
    const int py = (ty << p.tile_h_log2) + (lane >> p.tile_w_log2);
    const bool valid = px < p.width && py < p.height;
    const int cx = min(px, p.width - 1), cy = min(py, p.height - 1);
    const int64_t ray = (int64_t)cy * p.width + cx;

    float o[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = p.origins[ray * 3 + c];
        d[c] = p.directions[ray * 3 + c];
    }
    const float near = p.nears ? p.nears[ray] : p.near_plane;
    const float far = p.fars ? p.fars[ray] : p.far_plane;
    const float s_near = sn_spacing(near, su), s_far = sn_spacing(far, su);
    SnShOps sh;
    sh.build(d, p.sh_remap);

    const __amdgpu_buffer_rsrc_t rsrc = sn_table_rsrc(p.table, (16u << p.log2_t) * 8u);
    const int S = p.n_samples;
    const float* eb = nullptr;
    if (MODE == 1) eb = p.ebins + ((int64_t)(ty * p.tiles_x + tx) * (S + 1)) * 64 + lane;

    SnComposite comp;
    comp.init();
    auto bin = [&](int k) -> float {
        return MODE == 0 ? (shared_bins ? etab[k] : sn_euclid(p.sbins ? p.sbins[k] : (float)k / (float)S, s_near, s_far, su)) : eb[(int64_t)k * 64];
    };
    float t0 = bin(0);
    float r = 0.f, g = 0.f, b = 0.f;
#pragma unroll 1
    for (int i = 0; i < S; ++i) {
        asm volatile("" ::: "memory");  // keeps the loop-invariant LDS weight reads inside the loop (sn_render_main_kernel)
        const float t1 = bin(i + 1);
        float q[3];
        const bool sel = sn_sample_q(o, d, t0, t1, q, pm);
        float feat[32];
        sn_hash_encode<16, SN_HASH_GROUP, (GRID ? 2 : 1), -1>(rsrc, p.scal, p.log2_t, q, feat, &p.grid, &p.dense, nullptr, p.feat_scale);
        __builtin_amdgcn_sched_barrier(0);
        float h0, rgb[3];
        sn_wide_field_f32(lds, feat, sh, lane, h0, rgb);
        __builtin_amdgcn_sched_barrier(0);
        float density = p.avg_density * sn_exp<true>(h0) * (sel ? 1.0f : 0.0f);
        const float nan_term = fmaf(q[2], 0.0f, fmaf(q[1], 0.0f, q[0] * 0.0f));  // a NaN position stays NaN through the field (sn_render_main_kernel)
        density += nan_term;
        r = rgb[0] + nan_term;
        g = rgb[1] + nan_term;
        b = rgb[2] + nan_term;
        comp.step_fused(t0, t1, density, r, g, b);
        t0 = t1;
        // exact early termination of a saturated wave (sn_render_main_kernel): every later weight is exactly +0
        if (p.early_term && i < S - 2 && __all(comp.last_trans == 0.0f)) {
            i = S - 2;
            t0 = bin(S - 1);
        }
    }
    sn_main_epilogue<false>(p, comp, r, g, b, bin, S, valid, px, py, lane);
}

// rows a14/a15 on explicit world positions, wide field: sn_main_field_stage_kernel's contract, a grid-stride loop over blocks of 256
// points so that the 115 KB image is loaded once per workgroup
__global__ __launch_bounds__(256, 1) void sn_wide_field_stage_kernel(SnFieldStageParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    sn_wide_load_image(lds, p.wimg, tid);
    __syncthreads();
    const int lane = tid & 63;
    const __amdgpu_buffer_rsrc_t rsrc = sn_table_rsrc(p.table, (16u << p.log2_t) * 8u);
    const int64_t n_blocks = (p.n + 255) / 256;
#pragma unroll 1
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        asm volatile("" ::: "memory");
        const int64_t i = blk * 256 + tid;
        const int64_t j = i < p.n ? i : p.n - 1;
        const float pos[3] = {p.positions[j * 3], p.positions[j * 3 + 1], p.positions[j * 3 + 2]};
        float d[3] = {0.f, 0.f, 1.f};
        if (p.directions) {
            d[0] = p.directions[j * 3];
            d[1] = p.directions[j * 3 + 1];
            d[2] = p.directions[j * 3 + 2];
        }
        SnShOps sh;
        sh.build(d, p.sh_remap);
        float q[3];
        const bool sel = sn_position_q(pos, q, &p.pm);
        float feat[32];
        if (p.grid_mode) sn_hash_encode<16, 0, 2>(rsrc, p.scal, p.log2_t, q, feat, &p.grid);
        else sn_hash_encode<16>(rsrc, p.scal, p.log2_t, q, feat);
        __builtin_amdgcn_sched_barrier(0);
        float h0, rgb[3], geo16[16];
        sn_wide_field_f32<true>(lds, feat, sh, lane, h0, rgb, geo16);
        const bool qnan = (q[0] != q[0]) | (q[1] != q[1]) | (q[2] != q[2]);
        if (qnan) h0 = rgb[0] = rgb[1] = rgb[2] = __builtin_nanf("");
        if (i < p.n && p.geo) {
#pragma unroll
            for (int k = 0; k < 15; ++k) p.geo[i * 15 + k] = qnan ? __builtin_nanf("") : geo16[1 + k];
        }
        if (i < p.n) {
            p.density[i] = p.avg_density * expf(h0) * (sel ? 1.0f : 0.0f);
            if (p.rgb) {
                p.rgb[i * 3] = rgb[0];
                p.rgb[i * 3 + 1] = rgb[1];
                p.rgb[i * 3 + 2] = rgb[2];
            }
        }
    }
}
