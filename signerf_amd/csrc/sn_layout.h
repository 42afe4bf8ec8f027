// sn_layout.h -- layout of the weight images the host packs (sn_weights.h) and the kernels read (sn_main.h, sn_normals.h,
// sn_proposal.h), and the launch-shape constants the host plans with (sn_frame.h).  Constants only, plain C++: included by device and
// host-only code alike.
#pragma once

// LDS weight image of the main field, float offsets.  Built on the host by sn_weights.h
// (build_main_image, pack_main_images) -- keep the two in sync.
struct SnMainImg {
    static constexpr int W1 = 0;        // [rt=2][t4=4][lane=64][4]   32 -> 64
    static constexpr int W2 = 2048;     // [rt=1][t4=8][64][4]        64 -> 32 rows (16 real + dup)
    static constexpr int WC1 = 4096;    // [rt=2][t4=4][64][4]        (16 L2-rows + 16 SH) -> 64
    static constexpr int WC2 = 6144;    // [rt=2][t4=8][64][4]        64 -> 64
    static constexpr int B1 = 10240;    // [rt=2][h=2][16]
    static constexpr int B2 = 10304;    // [1][2][16]
    static constexpr int BC1 = 10336;   // [2][2][16]
    static constexpr int BC2 = 10400;   // [2][2][16]
    static constexpr int W3 = 10464;    // [n][h=2][32], n = 3 channels
    static constexpr int W3_ROWS = 3;
    static constexpr int B3 = W3 + W3_ROWS * 64;  // [4]: the 3 biases; [3] = 1 / (output scale of layer 2) of the split-precision image (h0 = row 0 * that)
    static constexpr int TOTAL = B3 + 4;  // 10 660 floats = 42 640 bytes; a multiple of 4
};

// LDS weight image of a WIDE main field (hidden_dim = hidden_dim_color = 128; sn_wide_kernels.h), float offsets, exact fp32 only.  Same
// operand orders as SnMainImg with four 32-row tiles per 128-wide layer and 64 k-steps per 128-wide input.  Built by sn_weights.h
// (build_wide_image).
struct SnWideImg {
    static constexpr int HIDDEN = 128;
    static constexpr int W1 = 0;         // [rt=4][t4=4][lane=64][4]    32 -> 128
    static constexpr int W2 = 4096;      // [rt=1][t4=16][64][4]        128 -> 32 rows (16 real + dup)
    static constexpr int WC1 = 8192;     // [rt=4][t4=4][64][4]         (16 L2-rows + 16 SH) -> 128
    static constexpr int WC2 = 12288;    // [rt=4][t4=16][64][4]        128 -> 128
    static constexpr int B1 = 28672;     // [rt=4][h=2][16]
    static constexpr int B2 = B1 + 128;  // [1][2][16]
    static constexpr int BC1 = B2 + 32;  // [4][2][16]
    static constexpr int BC2 = BC1 + 128;  // [4][2][16]
    static constexpr int W3 = BC2 + 128;   // [n=3][h=2][64]: colour layer 3 on the VALU, [rt*16 + r] <-> hidden rt*32 + rho(r) + 4h
    static constexpr int B3 = W3 + 3 * 128;  // [4]: the 3 biases
    static constexpr int TOTAL = B3 + 4;     // 29 476 floats = 117 904 bytes; a multiple of 4
    static constexpr int MAX_BINS = 1024 + 4;  // the uniform sampler's S + 1 euclidean bins behind the image (num_nerf_samples <= 1024)
};
static_assert(SnWideImg::TOTAL % 4 == 0, "the image is copied 16 bytes at a time");
static_assert((SnWideImg::TOTAL + SnWideImg::MAX_BINS) * 4 <= 160 * 1024, "wide image + bins table must fit the CU's 160 KiB LDS");

// byte offsets of the fp16x2 LDS image; weights [rt][s][hi|lo][lane][8 halves]
struct SnMainImgH {
    static constexpr int W1 = 0;          // 2 rt x 2 s x 2 x 1 KiB
    static constexpr int W2 = 8192;       // 1 x 4 x 2 KiB
    static constexpr int WC1 = 16384;     // 2 x 2 x 2 KiB
    static constexpr int WC2 = 24576;     // 2 x 4 x 2 KiB
    static constexpr int FP32 = 40960;    // then the fp32 tail, same sub-layout as SnMainImg from B1 on
    static constexpr int TAIL_FLOATS = SnMainImg::TOTAL - SnMainImg::B1;
    static constexpr int TOTAL_BYTES = FP32 + TAIL_FLOATS * 4;  // 42640
    static constexpr int B1 = 0, B2 = SnMainImg::B2 - SnMainImg::B1, BC1 = SnMainImg::BC1 - SnMainImg::B1,
                         BC2 = SnMainImg::BC2 - SnMainImg::B1, W3 = SnMainImg::W3 - SnMainImg::B1, B3 = SnMainImg::B3 - SnMainImg::B1;
};

// ReLU folded into the operand split of the main kernel (sn_main.h sn_split2_relu); the range conditioning of the host packers
// (sn_weights.h plan_split_scales) keeps every pre-activation below the 2^10 that fold needs.
#ifndef SN_RELU_FOLD
#define SN_RELU_FOLD 1
#endif

// single-fp16 form of the main field (sn_main.h "Single-fp16 form"): colour layer 3's fp16 A operand behind the split-precision image
struct SnMainImgF16 {
    static constexpr int W3H = SnMainImg::TOTAL * 4;   // byte offset: A operand of colour layer 3, [s = 4][lane = 64][8 halves], rows 0..2 real
    static constexpr int TAILF = W3H + 4096;           // float[4]: [0] = 1 / s5 (the power-of-two scale of that operand)
    static constexpr int TOTAL_BYTES = TAILF + 16;
    static constexpr int TOTAL_FLOATS = TOTAL_BYTES / 4;
};

struct SnNormImg {  // float offsets.  [0, SnMainImg::TOTAL) has SnMainImg's layout, the pred-normal MLP in the colour slots
    static constexpr int WB = SnMainImg::TOTAL;  // [rt=1][t4=8][64][4]: mask (64, layer-1 output order) -> d h0 / d feat (32 rows)
    static constexpr int ZB = WB + 2048;         // its bias image: 32 zeros
    static constexpr int TOTAL = ZB + 32;        // 12 740 floats = 50 960 B
};

// fp16x2 form: SnMainImgH (pred-normal MLP in the colour slots) followed by the reverse-pass layer in the same operand order
struct SnNormImgH {
    static constexpr int WB = SnMainImgH::TOTAL_BYTES;  // [s=4][hi|lo][lane][8 halves] = 8 KiB
    static constexpr int TOTAL_BYTES = WB + 8192;       // 50 832
};

// proposal-net MLP pack (floats): W0 [k=10][n=16] (k-major), b0 [16], W1 [16], b1
#define SN_PROP_W0 0
#define SN_PROP_B0 160
#define SN_PROP_W1 176
#define SN_PROP_B1 192
// ... followed by the matrix-core form of the same weights (SN_PROP_MFMA): two A operands of v_mfma_f32_32x32x16_f16 as fp16 hi / lo
// parts, [lane][8 halves] each (sn_proposal.h sn_prop_mlp_mfma: rows 0..15 serve the rays of lanes 0..31 through k = 0..7, rows 16..31 the
// rays of lanes 32..63 through k = 8..15), and the layer-2 weights in accumulator order, [h][r] = W1[(r & 3) + 8 (r >> 2) + 4 h], r = 0..7
#define SN_PROP_MA1_HI 196
#define SN_PROP_MA1_LO 452
#define SN_PROP_MA2_HI 708
#define SN_PROP_MA2_LO 964
#define SN_PROP_MW1 1220
// ... and the linear half of layer 2 (sn_prop_mlp_mfma): [k < 10] = sum_r W1[r] W0[r][k] / 2 (per unit of the SCALED features), [10] =
// sum_r W1[r] b0[r] / 2 + b1
#define SN_PROP_LIN 1236
#define SN_PROP_PACK_FLOATS 1252

// Launch shapes the host plans with (sn_frame.h) and the kernels are compiled for.
// the occupancy the main kernel is compiled for (168 VGPRs): workgroups of 4 waves per CU
#ifndef SN_MAIN_WAVES_PER_SIMD
#define SN_MAIN_WAVES_PER_SIMD 3
#endif
#define SN_PROP_MAX_SAMPLES 256
#define SN_PROP_WAVES 4
#ifndef SN_PROP_WG_PER_CU
#define SN_PROP_WG_PER_CU 3  // = waves per SIMD the kernel is compiled for (<= 168 VGPRs)
#endif
// per-wave scratch of the proposal kernel: weights [256][64] + two spacing-bin arrays [257][64]
#define SN_PROP_SCRATCH_W 0
#define SN_PROP_SCRATCH_B0 (SN_PROP_MAX_SAMPLES * 64)
#define SN_PROP_SCRATCH_B1 (SN_PROP_SCRATCH_B0 + (SN_PROP_MAX_SAMPLES + 1) * 64)
#define SN_PROP_SCRATCH_FLOATS (SN_PROP_SCRATCH_B1 + (SN_PROP_MAX_SAMPLES + 1) * 64)
