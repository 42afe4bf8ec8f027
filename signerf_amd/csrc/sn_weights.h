// sn_weights.h -- host-side packers of the weight images: everything sn_finalize_weights computes from the uploaded parameter
// tensors before it touches the device.  Plain C++17, no HIP: tests/c/weights_pack.cpp compiles this header alone and
// tests/test_weights_host.py holds its output, byte for byte, against digests recorded from the device (tests/golden/weight_images.json).
// The operand orders written here (rho, the (t, h) and (s, h, e) k-slot maps) are the ones the kernels of sn_main.h, sn_normals.h and
// sn_proposal.h read; the offsets both sides share live in sn_layout.h.
#pragma once
#include "../../include/signerf_hip.h"
#include "sn_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

inline int rho(int r) { return (r & 3) + 8 * (r >> 2); }

// Host-side construction of the LDS weight image consumed by sn_main_field_f32 (sn_main.h; offsets: sn_layout.h).
// W1 [64,32], b1 [64]; W2 [16,64], b2 [16]; Wc1 [64,63], bc1 [64]; Wc2 [64,64], bc2; Wc3 [3,64], bc3 [3];
// app [A] = mean appearance embedding (folded into the colour-layer-1 bias; A14).
inline std::vector<float> build_main_image(const SnFieldDesc& d, const float* W1, const float* b1, const float* W2, const float* b2,
                                    const float* Wc1, const float* bc1, const float* Wc2, const float* bc2, const float* Wc3,
                                    const float* bc3, const float* app) {
    std::vector<float> img(SnMainImg::TOTAL, 0.0f);
    const int geo = d.geo_feat_dim;           // 15
    const int sh = d.sh_levels * d.sh_levels;  // 16
    const int cin = sh + geo + d.appearance_embed_dim;
    auto put = [&](int base, int KS, int rt, int t, int lane, float v) {
        img[base + ((rt * (KS / 4) + t / 4) * 64 + lane) * 4 + (t % 4)] = v;
    };
    // layer 1: slot (t,h) <-> feature 2t+h
    for (int rt = 0; rt < 2; ++rt)
        for (int t = 0; t < 16; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                int row = rt * 32 + (lane & 31), h = lane >> 5;
                put(SnMainImg::W1, 16, rt, t, lane, W1[row * 32 + 2 * t + h]);
            }
    // layer 2: 32 padded rows: 0 = h0, 1..15 = geo, 20 = h0 again (so that lanes 32-63 find their
    // sample's density in their own half), rest zero.  slot (t = rt'*16 + r, h) <-> hidden rt'*32 + rho(r) + 4h
    auto l2src = [&](int row) { return row < 16 ? row : (row == 20 ? 0 : -1); };
    for (int t = 0; t < 32; ++t)
        for (int lane = 0; lane < 64; ++lane) {
            int row = lane & 31, h = lane >> 5, src = l2src(row);
            int hid = (t / 16) * 32 + rho(t % 16) + 4 * h;
            put(SnMainImg::W2, 32, 0, t, lane, src >= 0 ? W2[src * 64 + hid] : 0.0f);
        }
    // colour layer 1: k-steps 0..7 <- layer-2 rows rho(t)+4h (row 0 = h0 is not an input; rows 1..15 = geo 0..14
    // = colour inputs sh+0 .. sh+14); k-steps 8..15 <- SH component 2(t-8)+h = colour input 2(t-8)+h
    for (int rt = 0; rt < 2; ++rt)
        for (int t = 0; t < 16; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                int row = rt * 32 + (lane & 31), h = lane >> 5;
                float v = 0.0f;
                if (t < 8) {
                    int l2row = rho(t) + 4 * h;
                    if (l2row >= 1 && l2row <= geo) v = Wc1[row * cin + sh + (l2row - 1)];
                } else {
                    int s = 2 * (t - 8) + h;
                    if (s < sh) v = Wc1[row * cin + s];
                }
                put(SnMainImg::WC1, 16, rt, t, lane, v);
            }
    // colour layer 2
    for (int rt = 0; rt < 2; ++rt)
        for (int t = 0; t < 32; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                int row = rt * 32 + (lane & 31), h = lane >> 5;
                int hid = (t / 16) * 32 + rho(t % 16) + 4 * h;
                put(SnMainImg::WC2, 32, rt, t, lane, Wc2[row * 64 + hid]);
            }
    // bias images [rt][h][r] -> bias[rt*32 + rho(r) + 4h]
    auto bias_img = [&](int base, int RT, auto&& f) {
        for (int rt = 0; rt < RT; ++rt)
            for (int h = 0; h < 2; ++h)
                for (int r = 0; r < 16; ++r) img[base + (rt * 2 + h) * 16 + r] = f(rt * 32 + rho(r) + 4 * h);
    };
    bias_img(SnMainImg::B1, 2, [&](int n) { return b1[n]; });
    bias_img(SnMainImg::B2, 1, [&](int row) {
        int src = l2src(row);
        return src >= 0 ? b2[src] : 0.0f;
    });
    bias_img(SnMainImg::BC1, 2, [&](int n) {
        float acc = bc1[n];
        for (int a = 0; a < d.appearance_embed_dim; ++a) acc += Wc1[n * cin + sh + geo + a] * app[a];
        return acc;
    });
    bias_img(SnMainImg::BC2, 2, [&](int n) { return bc2[n]; });
    // colour layer 3 (VALU): [n][h][rt*16 + r] = Wc3[n][rt*32 + rho(r) + 4h]
    for (int n = 0; n < 3; ++n)
        for (int h = 0; h < 2; ++h)
            for (int rt = 0; rt < 2; ++rt)
                for (int r = 0; r < 16; ++r)
                    img[SnMainImg::W3 + (n * 2 + h) * 32 + rt * 16 + r] = Wc3[n * 64 + rt * 32 + rho(r) + 4 * h];
    for (int n = 0; n < 3; ++n) img[SnMainImg::B3 + n] = bc3[n];
    return img;
}


// ---- fp16 helpers (host) -------------------------------------------------------------------------------------
inline uint16_t f32_to_f16_rne(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7bffu);  // saturate instead of inf (matches cvt_pkrtz on the device side)
    if (x < 0x38800000u) {                                     // subnormal half (or zero)
        if (x < 0x33000000u) return (uint16_t)sign;
        const int shift = 126 - (int)(x >> 23);                // 14..24
        uint32_t mant = (x & 0x7fffffu) | 0x800000u;
        uint32_t half = mant >> shift;
        const uint32_t rem = mant & ((1u << shift) - 1u), mid = 1u << (shift - 1);
        if (rem > mid || (rem == mid && (half & 1u))) ++half;
        return (uint16_t)(sign | half);
    }
    uint32_t half = ((x - 0x38000000u) >> 13);
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (half & 1u))) ++half;
    return (uint16_t)(sign | half);
}

inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu, x;
    if (e == 0) {
        if (m == 0) x = sign;
        else {
            int sh = 0;
            while (!(m & 0x400u)) { m <<= 1; ++sh; }
            x = sign | ((uint32_t)(113 - sh) << 23) | ((m & 0x3ffu) << 13);
        }
    } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
    else x = sign | ((e + 112) << 23) | (m << 13);
    float f;
    memcpy(&f, &x, 4);
    return f;
}

// fp16x2 LDS image consumed by sn_main_field_h: same rows / folded bias as build_main_image, other k-slot order.
inline std::vector<float> build_main_image_h(const SnFieldDesc& d, const float* W1, const float* W2, const float* Wc1, const float* Wc2,
                                      const std::vector<float>& img32) {
    std::vector<float> out(SnMainImg::TOTAL, 0.0f);
    uint16_t* hw = (uint16_t*)out.data();
    const int geo = d.geo_feat_dim, sh = d.sh_levels * d.sh_levels, cin = sh + geo + d.appearance_embed_dim;
    auto put = [&](int base_bytes, int KS, int rt, int s, int lane, int e, float w) {
        const uint16_t hi = f32_to_f16_rne(w);
        const uint16_t lo = f32_to_f16_rne(w - f16_to_f32(hi));
        const size_t off = (size_t)base_bytes / 2 + ((size_t)((rt * KS + s) * 2) * 64 + lane) * 8 + e;
        hw[off] = hi;
        hw[off + 512] = lo;  // the lo plane follows 64 lanes x 8 halves later
    };
    auto l2src = [&](int row) { return row < 16 ? row : (row == 20 ? 0 : -1); };
    for (int lane = 0; lane < 64; ++lane) {
        const int h = lane >> 5, i = lane & 31;
        for (int e = 0; e < 8; ++e) {
            for (int rt = 0; rt < 2; ++rt)
                for (int s = 0; s < 2; ++s) put(SnMainImgH::W1, 2, rt, s, lane, e, W1[(rt * 32 + i) * 32 + 16 * s + 8 * h + e]);
            for (int s = 0; s < 4; ++s) {  // hidden unit of slot (s = 2 rt' + s', h, e): rt'*32 + rho(8 s' + e) + 4h
                const int hid = (s / 2) * 32 + rho(8 * (s % 2) + e) + 4 * h, src = l2src(i);
                put(SnMainImgH::W2, 4, 0, s, lane, e, src >= 0 ? W2[src * 64 + hid] : 0.0f);
                for (int rt = 0; rt < 2; ++rt) put(SnMainImgH::WC2, 4, rt, s, lane, e, Wc2[(rt * 32 + i) * 64 + hid]);
            }
            for (int rt = 0; rt < 2; ++rt) {
                const int row = rt * 32 + i;
                const int l2row = rho(e) + 4 * h;  // k-step 0: layer-2 rows
                put(SnMainImgH::WC1, 2, rt, 0, lane, e, (l2row >= 1 && l2row <= geo) ? Wc1[row * cin + sh + (l2row - 1)] : 0.0f);
                const int comp = 8 * h + e;        // k-step 1: SH components
                put(SnMainImgH::WC1, 2, rt, 1, lane, e, comp < sh ? Wc1[row * cin + comp] : 0.0f);
            }
        }
    }
    memcpy((char*)out.data() + SnMainImgH::FP32, img32.data() + SnMainImg::B1, (size_t)SnMainImgH::TAIL_FLOATS * 4);
    return out;
}

// ---- range conditioning of the split-precision MLPs ---------------------------------------------------------------------------
// Every fp32 operand of the "fp16x2" path is carried as fp16 hi + lo.  That is fp32-grade (2^-22 relative) only while the operand sits
// in [2^-3, 65504]: below, lo drops into fp16's subnormals (absolute resolution 2^-24, e.g. ~13 bits for a value of 5e-4 -- nerfstudio
// initialises its tables at 1e-3); above, cvt_pkrtz saturates.  Scaling by a power of two is exact, so pack_main_images moves
// every layer into the upper part of the range once, on the host, at no run-time cost:
//   features   f' = t0 f        t0 = 2^floor(log2(2^10 / max|table|)); the de-hashed copies / paired tables store t0 * row (levels read
//                               from the uploaded table are multiplied in the kernel), the first layer's weights carry 1 / t0
//   layer l    z_l' = s_l z_l   s_l = 2^floor(log2(2^10 / B_l)), B_l = interval bound of |z_l| over all inputs with |f| <= max|table|;
//                               W_l' = W_l s_l / s_(l-1), b_l' = b_l s_l; ReLU commutes with s_l > 0; the last consumer divides it out
// B_l is a true bound, so no activation can saturate; the largest weights of a layer land in [2^-1, 2^4] by construction.  The only
// failure left is a scaled weight outside the fp16 range (a unit whose inputs are bounded ~0 next to ordinary ones): the handle then
// renders precision-1 requests with the exact fp32 MFMA path (sn_effective_precision reports it).
inline float pow2_floor(double x) {
    if (!(x > 0.0) || !std::isfinite(x)) return 1.0f;
    // exponent clamped to +-80: scales stay finite fp32 numbers with finite products and reciprocals whatever the parameters are
    // (a table whose largest entry is below 2^-70 is a zero field for every practical purpose)
    return (float)std::ldexp(1.0, std::max(-80, std::min(80, (int)std::floor(std::log2(x)))));
}

struct MainSplitPlan {
    float t0 = 1.0f, s1 = 1.0f, s2 = 1.0f, s3 = 1.0f, s4 = 1.0f;
    bool ok = true;
    std::string why;
    double max_bound = 0.0;  // largest interval bound of an (unscaled) activation
    double B2[16] = {};      // interval bounds of the (unscaled) layer-2 outputs: row 0 = h0, rows 1..15 = the geo features
};

inline MainSplitPlan plan_split_scales(const SnFieldDesc& d, float table_absmax, bool scale_features, const float* W1, const float* b1, const float* W2,
                                const float* b2, const float* Wc1, const float* bc1, const float* Wc2, const float* bc2, const float* app) {
    MainSplitPlan pl;
    const int geo = d.geo_feat_dim, sh = d.sh_levels * d.sh_levels, cin = sh + geo + d.appearance_embed_dim;
    if (!std::isfinite(table_absmax)) {
        pl.ok = false;
        pl.why = "the hash table holds non-finite values";
        return pl;
    }
    const double M0 = table_absmax;
    pl.t0 = scale_features && M0 > 0.0 ? pow2_floor(1024.0 / M0) : 1.0f;
    std::vector<double> B1(64), B2(16), Bc1(64), Bc2(64);
    double m1 = 0, m2 = 0, m3 = 0, m4 = 0;
    for (int n = 0; n < 64; ++n) {
        double a = std::fabs(b1[n]);
        for (int k = 0; k < 32; ++k) a += std::fabs(W1[n * 32 + k]) * M0;
        B1[n] = a;
        m1 = std::max(m1, a);
    }
    for (int r = 0; r < 16; ++r) {
        double a = std::fabs(b2[r]);
        for (int n = 0; n < 64; ++n) a += std::fabs(W2[r * 64 + n]) * B1[n];
        B2[r] = a;
        pl.B2[r] = a;
        m2 = std::max(m2, a);
    }
    for (int n = 0; n < 64; ++n) {
        double a = std::fabs(bc1[n]);
        for (int e = 0; e < d.appearance_embed_dim; ++e) a += std::fabs(Wc1[n * cin + sh + geo + e] * app[e]);
        for (int c = 0; c < sh; ++c) a += std::fabs(Wc1[n * cin + c]) * 3.0;  // |SH component| < 3 for degree 4 on [-1, 1]^3
        for (int j = 0; j < geo; ++j) a += std::fabs(Wc1[n * cin + sh + j]) * B2[1 + j];
        Bc1[n] = a;
        m3 = std::max(m3, a);
    }
    for (int n = 0; n < 64; ++n) {
        double a = std::fabs(bc2[n]);
        for (int k = 0; k < 64; ++k) a += std::fabs(Wc2[n * 64 + k]) * Bc1[k];
        Bc2[n] = a;
        m4 = std::max(m4, a);
    }
    if (!std::isfinite(m1) || !std::isfinite(m2) || !std::isfinite(m3) || !std::isfinite(m4)) {
        pl.ok = false;
        pl.why = "non-finite MLP parameters";
        return pl;
    }
    pl.max_bound = std::max(std::max(m1, m2), std::max(m3, m4));
    // target: every scaled pre-activation below 2^10 -- far inside fp16's range, and below 2048, which the ReLU folded into the operand
    // split needs (sn_main.h sn_split2_relu: the low part a - RTZ16(a) must stay below 1 for its clamp to be a plain max(., 0))
    const double target = SN_RELU_FOLD ? 1024.0 : 16384.0;
    pl.s1 = m1 > 0 ? pow2_floor(target / m1) : 1.0f;
    pl.s2 = m2 > 0 ? pow2_floor(target / m2) : 1.0f;
    pl.s3 = m3 > 0 ? pow2_floor(target / m3) : 1.0f;
    pl.s4 = m4 > 0 ? pow2_floor(target / m4) : 1.0f;
    return pl;
}

// true if every element of a scaled operand fits fp16 (|x| <= 65504) -- the split saturates beyond
inline bool fits_half(const std::vector<float>& v) {
    for (float x : v)
        if (!(std::fabs(x) <= 65504.0f)) return false;
    return true;
}

// v * f per element; f is a power of two wherever the packers use it: exact (barring under / overflow)
inline std::vector<float> scaled(const std::vector<float>& v, double f) {
    std::vector<float> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = (float)((double)v[i] * f);
    return o;
}

// ---- main field ---------------------------------------------------------------------------------------------------------------
// W1 [64,32], b1 [64]; W2 [16,64], b2 [16]; Wc1 [64,cin], bc1 [64]; Wc2 [64,64], bc2 [64]; Wc3 [3,64], bc3 [3]; app [A] = mean appearance
// embedding (all zero when the field has none); cin = sh_levels^2 + geo_feat_dim + A
struct SnMainTensors {
    const std::vector<float>*W1, *b1, *W2, *b2, *Wc1, *bc1, *Wc2, *bc2, *Wc3, *bc3, *app;
};

struct SnMainImages {
    std::vector<float> img;   // SnMainImg: exact fp32, W1 / t0
    std::vector<float> imgh;  // SnMainImgH followed by the SnMainImgF16 tail: every layer in its conditioned range
    MainSplitPlan plan;       // plan.t0 = the feature scale the de-hashed copies and paired tables carry
    bool split_ok = true;     // false: some scaled weight leaves the fp16 range (or the plan failed): split_why says which
    std::string split_why;
    std::vector<float> W1s, b1s, W2s, b2s;  // the conditioned density MLP, shared with the normals images
};

inline SnMainImages pack_main_images(const SnFieldDesc& d, const SnMainTensors& p, float table_absmax) {
    SnMainImages out;
    const int cin = d.sh_levels * d.sh_levels + d.geo_feat_dim + d.appearance_embed_dim;
    const MainSplitPlan pl = plan_split_scales(d, table_absmax, true, p.W1->data(), p.b1->data(), p.W2->data(), p.b2->data(), p.Wc1->data(),
                                               p.bc1->data(), p.Wc2->data(), p.bc2->data(), p.app->data());
    out.split_ok = pl.ok;
    out.split_why = pl.why;
    // exact-fp32 image: only the feature scale (the de-hashed copies carry it), W1 / t0 -- bit-identical results
    const std::vector<float> W1f = scaled(*p.W1, 1.0 / pl.t0);
    out.img = build_main_image(d, W1f.data(), p.b1->data(), p.W2->data(), p.b2->data(), p.Wc1->data(), p.bc1->data(),
                               p.Wc2->data(), p.bc2->data(), p.Wc3->data(), p.bc3->data(), p.app->data());
    // split-precision image: every layer in its conditioned range (plan_split_scales)
    const int sh_n = d.sh_levels * d.sh_levels;
    out.W1s = scaled(*p.W1, (double)pl.s1 / pl.t0);
    out.b1s = scaled(*p.b1, pl.s1);
    out.W2s = scaled(*p.W2, (double)pl.s2 / pl.s1);
    out.b2s = scaled(*p.b2, pl.s2);
    const std::vector<float>&W1s = out.W1s, &b1s = out.b1s, &W2s = out.W2s, &b2s = out.b2s;
    std::vector<float> Wc1s = scaled(*p.Wc1, pl.s3);  // SH and appearance columns; the geo columns take s3 / s2
    for (int n = 0; n < 64; ++n)
        for (int j = 0; j < d.geo_feat_dim; ++j) Wc1s[(size_t)n * cin + sh_n + j] = (float)((double)(*p.Wc1)[(size_t)n * cin + sh_n + j] * ((double)pl.s3 / pl.s2));
    const std::vector<float> bc1s = scaled(*p.bc1, pl.s3);
    const std::vector<float> Wc2s = scaled(*p.Wc2, (double)pl.s4 / pl.s3), bc2s = scaled(*p.bc2, pl.s4);
    const std::vector<float> Wc3s = scaled(*p.Wc3, 1.0 / pl.s4);
    if (out.split_ok && !(fits_half(W1s) && fits_half(W2s) && fits_half(Wc1s) && fits_half(Wc2s))) {
        out.split_ok = false;
        out.split_why = "a range-conditioned MLP weight leaves the fp16 range";
    }
    std::vector<float> img_s = build_main_image(d, W1s.data(), b1s.data(), W2s.data(), b2s.data(), Wc1s.data(), bc1s.data(), Wc2s.data(),
                                                bc2s.data(), Wc3s.data(), p.bc3->data(), p.app->data());
    img_s[SnMainImg::B3 + 3] = 1.0f / pl.s2;
    out.imgh = build_main_image_h(d, W1s.data(), W2s.data(), Wc1s.data(), Wc2s.data(), img_s);
    {
        // single-fp16 mode (sn_main.h SnMainImgF16): colour layer 3 as an fp16 A operand behind the image -- rows 0..2 = the three output
        // channels, k-slot (s, h, e) <-> hidden unit (s / 2) 32 + rho(8 (s % 2) + e) + 4 h (the operand order colour layer 2's output is
        // converted into), lifted by the power of two s5 so that its largest entry sits in [128, 256) (the weights already carry 1 / s4)
        out.imgh.resize(SnMainImgF16::TOTAL_FLOATS, 0.0f);
        double m = 0.0;
        for (float w : Wc3s) m = std::max(m, (double)std::fabs(w));
        const float s5 = m > 0 && std::isfinite(m) ? pow2_floor(256.0 / m) : 1.0f;
        uint16_t* hw = (uint16_t*)((char*)out.imgh.data() + SnMainImgF16::W3H);
        for (int sk = 0; sk < 4; ++sk)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int row = lane & 31, hh = lane >> 5;
                    const int hid = (sk / 2) * 32 + rho(8 * (sk % 2) + e) + 4 * hh;
                    hw[((size_t)sk * 64 + lane) * 8 + e] = row < 3 ? f32_to_f16_rne((float)((double)Wc3s[row * 64 + hid] * s5)) : (uint16_t)0;
                }
        *(float*)((char*)out.imgh.data() + SnMainImgF16::TAILF) = 1.0f / s5;
    }
    out.plan = pl;
    return out;
}

// ---- wide main field (hidden_dim = hidden_dim_color = 128) ----------------------------------------------------------------------
// The LDS image consumed by sn_wide_field_tile (sn_wide_kernels.h; offsets: sn_layout.h SnWideImg), exact fp32, no range conditioning
// and no feature scale (a wide handle reads the uploaded table only).  Same operand orders as build_main_image:
//   A operand of k-step t, lane (i = lane & 31, h = lane >> 5), row tile rt  <->  W[rt*32 + i][k(t, h)]
//   k(t, h) of a 32-wide input (layer 1):        feature 2t + h
//   k(t, h) of a 128-wide input (t = 0..63):     hidden unit (t/16)*32 + rho(t%16) + 4h   (the accumulator order of the layer before)
//   colour layer 1: k-steps 0..7 <- layer-2 rows rho(t) + 4h (row 0 = h0 is no input), k-steps 8..15 <- SH component 2(t-8) + h
// W1 [128,32], b1 [128]; W2 [16,128], b2 [16]; Wc1 [128,cin], bc1 [128]; Wc2 [128,128], bc2 [128]; Wc3 [3,128], bc3 [3]; app [A].
inline std::vector<float> build_wide_image(const SnFieldDesc& d, const float* W1, const float* b1, const float* W2, const float* b2,
                                           const float* Wc1, const float* bc1, const float* Wc2, const float* bc2, const float* Wc3,
                                           const float* bc3, const float* app) {
    constexpr int H = SnWideImg::HIDDEN, RT = H / 32, KH = H / 2;  // 4 row tiles, 64 k-steps over a 128-wide input
    std::vector<float> img(SnWideImg::TOTAL, 0.0f);
    const int geo = d.geo_feat_dim;            // 15
    const int sh = d.sh_levels * d.sh_levels;  // 16
    const int cin = sh + geo + d.appearance_embed_dim;
    auto put = [&](int base, int KS, int rt, int t, int lane, float v) {
        img[base + ((rt * (KS / 4) + t / 4) * 64 + lane) * 4 + (t % 4)] = v;
    };
    auto hid_of = [](int t, int h) { return (t / 16) * 32 + rho(t % 16) + 4 * h; };
    auto l2src = [&](int row) { return row < 16 ? row : (row == 20 ? 0 : -1); };  // row 20 repeats h0 for the upper half-wave
    for (int lane = 0; lane < 64; ++lane) {
        const int i = lane & 31, h = lane >> 5;
        for (int rt = 0; rt < RT; ++rt) {
            const int row = rt * 32 + i;
            for (int t = 0; t < 16; ++t) {
                put(SnWideImg::W1, 16, rt, t, lane, W1[row * 32 + 2 * t + h]);
                float v = 0.0f;
                if (t < 8) {
                    const int l2row = rho(t) + 4 * h;
                    if (l2row >= 1 && l2row <= geo) v = Wc1[(size_t)row * cin + sh + (l2row - 1)];
                } else {
                    const int s = 2 * (t - 8) + h;
                    if (s < sh) v = Wc1[(size_t)row * cin + s];
                }
                put(SnWideImg::WC1, 16, rt, t, lane, v);
            }
            for (int t = 0; t < KH; ++t) put(SnWideImg::WC2, KH, rt, t, lane, Wc2[row * H + hid_of(t, h)]);
        }
        for (int t = 0; t < KH; ++t) {
            const int src = l2src(i);
            put(SnWideImg::W2, KH, 0, t, lane, src >= 0 ? W2[src * H + hid_of(t, h)] : 0.0f);
        }
    }
    // bias images [rt][h][r] -> bias[rt*32 + rho(r) + 4h]
    auto bias_img = [&](int base, int nrt, auto&& f) {
        for (int rt = 0; rt < nrt; ++rt)
            for (int h = 0; h < 2; ++h)
                for (int r = 0; r < 16; ++r) img[base + (rt * 2 + h) * 16 + r] = f(rt * 32 + rho(r) + 4 * h);
    };
    bias_img(SnWideImg::B1, RT, [&](int n) { return b1[n]; });
    bias_img(SnWideImg::B2, 1, [&](int row) {
        const int src = l2src(row);
        return src >= 0 ? b2[src] : 0.0f;
    });
    bias_img(SnWideImg::BC1, RT, [&](int n) {  // the mean appearance embedding is a constant input: folded into the bias (A14)
        float acc = bc1[n];
        for (int a = 0; a < d.appearance_embed_dim; ++a) acc += Wc1[(size_t)n * cin + sh + geo + a] * app[a];
        return acc;
    });
    bias_img(SnWideImg::BC2, RT, [&](int n) { return bc2[n]; });
    for (int n = 0; n < 3; ++n)
        for (int h = 0; h < 2; ++h)
            for (int rt = 0; rt < RT; ++rt)
                for (int r = 0; r < 16; ++r) img[SnWideImg::W3 + (n * 2 + h) * (H / 2) + rt * 16 + r] = Wc3[n * H + rt * 32 + rho(r) + 4 * h];
    for (int n = 0; n < 3; ++n) img[SnWideImg::B3 + n] = bc3[n];
    return img;
}

// true for the descriptor of a wide field: both MLPs of the main field are 128 wide (sn_create refuses mixed pairs)
inline bool sn_is_wide(const SnFieldDesc& d) { return d.main_field.hidden_dim == SnWideImg::HIDDEN && d.hidden_dim_color == SnWideImg::HIDDEN; }

inline std::vector<float> pack_wide_image(const SnFieldDesc& d, const SnMainTensors& p) {
    return build_wide_image(d, p.W1->data(), p.b1->data(), p.W2->data(), p.b2->data(), p.Wc1->data(), p.bc1->data(), p.Wc2->data(),
                            p.bc2->data(), p.Wc3->data(), p.bc3->data(), p.app->data());
}

// ---- normals ------------------------------------------------------------------------------------------------------------------
// the pred-normal MLP w0 [64,12+geo], c0 [64]; w1 [64,64], c1 [64]; w2 [64,64], c2 [64] and its head wh [3,64], ch [3]: all or none
struct SnPredNormalTensors {
    const std::vector<float>*w0 = nullptr, *c0 = nullptr, *w1 = nullptr, *c1 = nullptr, *w2 = nullptr, *c2 = nullptr, *wh = nullptr, *ch = nullptr;
    bool complete() const { return w0 && c0 && w1 && c1 && w2 && c2 && wh && ch; }
};

struct SnNormalImages {
    std::vector<float> nimg;  // SnNormImg
    std::vector<float> nh;    // SnNormImgH
    bool has_pred_normals = false;
    bool normals_split_ok = true;     // the normals kernel's own conditioned operands fit fp16
    float grad_scale_normals = 1.0f;  // power of two carried by the split-precision reverse-pass layer
};

inline SnNormalImages pack_normal_images(const SnFieldDesc& d, const SnMainTensors& p, const SnMainImages& main, const SnPredNormalTensors& pn) {
    SnNormalImages out;
    const MainSplitPlan& pl = main.plan;
    const std::vector<float>&W1s = main.W1s, &b1s = main.b1s, &W2s = main.W2s, &b2s = main.b2s;
    const int pin = 12 + d.geo_feat_dim;
    // Normals image (sn_normals.h): the density MLP of the main image, the pred-normal MLP (if uploaded) in the colour slots,
    // and the transposed layer of the reverse pass.  The pred-normal MLP's last linear layer (64 -> 64, no activation) and
    // PredNormalsFieldHead's Linear(64 -> 3) are multiplied together here.
    out.has_pred_normals = pn.complete();
    SnFieldDesc dn = d;
    dn.appearance_embed_dim = 0;
    const int sh = d.sh_levels * d.sh_levels, cin_n = sh + d.geo_feat_dim;
    std::vector<float> P1((size_t)64 * cin_n, 0.0f), z64(64, 0.0f), z6464(64 * 64, 0.0f), Wf(3 * 64, 0.0f), bf(3, 0.0f);
    if (out.has_pred_normals) {
        for (int n = 0; n < 64; ++n) {
            for (int k = 0; k < 12; ++k) P1[(size_t)n * cin_n + k] = (*pn.w0)[(size_t)n * pin + k];  // position encoding -> SH slots
            for (int k = 0; k < d.geo_feat_dim; ++k) P1[(size_t)n * cin_n + sh + k] = (*pn.w0)[(size_t)n * pin + 12 + k];
        }
        for (int n = 0; n < 3; ++n) {
            double b = (*pn.ch)[n];
            for (int j = 0; j < 64; ++j) b += (double)(*pn.wh)[n * 64 + j] * (double)(*pn.c2)[j];
            bf[n] = (float)b;
            for (int k = 0; k < 64; ++k) {
                double a = 0.0;
                for (int j = 0; j < 64; ++j) a += (double)(*pn.wh)[n * 64 + j] * (double)(*pn.w2)[j * 64 + k];
                Wf[n * 64 + k] = (float)a;
            }
        }
    }
    out.nimg = build_main_image(dn, p.W1->data(), p.b1->data(), p.W2->data(), p.b2->data(), P1.data(),
                                               out.has_pred_normals ? pn.c0->data() : z64.data(),
                                               out.has_pred_normals ? pn.w1->data() : z6464.data(),
                                               out.has_pred_normals ? pn.c1->data() : z64.data(), Wf.data(), bf.data(), nullptr);
    out.nimg.resize(SnNormImg::TOTAL, 0.0f);
    // reverse pass: row f <- sum over hidden j of W1[j][f] * W2[0][j] * mask_j; slot (t, h) <-> hidden (t/16)*32 + rho(t%16) + 4h
    for (int t32 = 0; t32 < 32; ++t32)
        for (int lane = 0; lane < 64; ++lane) {
            const int f = lane & 31, hh = lane >> 5;
            const int hid = (t32 / 16) * 32 + rho(t32 % 16) + 4 * hh;
            out.nimg[SnNormImg::WB + ((t32 / 4) * 64 + lane) * 4 + (t32 % 4)] = (*p.W1)[hid * 32 + f] * (*p.W2)[hid];
        }
    // fp16 hi+lo form, RANGE-CONDITIONED like the main image (r03; r02 split the unconditioned matrices and fell back to exact fp32
    // as soon as max|table| < 1/8 -- i.e. for every real checkpoint: nerfstudio initialises its tables at 1e-3, tiny-cuda-nn at
    // 1e-4).  The density MLP's layers are the main image's (W1 s1 / t0, b1 s1, W2 s2 / s1, b2 s2: features come in times t0, h0
    // leaves through the 1 / s2 slot); the pred-normal MLP gets its own output scales from interval bounds over |pe| <= 1 and the
    // geo bounds B2: layer 1 -> s3n, layer 2 -> s4n, the fp32 (layer 3 . head) weights carry 1 / s4n; the reverse-pass layer
    // W1^T diag(W2[0,:]) is lifted by gsc so that its largest entry sits at ~2^10.
    const double tgt = SN_RELU_FOLD ? 1024.0 : 16384.0;
    double m3n = 0.0, m4n = 0.0, mwb = 0.0;
    std::vector<double> Bp1(64, 0.0);
    if (out.has_pred_normals) {
        for (int n = 0; n < 64; ++n) {
            double a = std::fabs((*pn.c0)[n]);
            for (int k = 0; k < 12; ++k) a += std::fabs((*pn.w0)[(size_t)n * pin + k]);
            for (int j = 0; j < d.geo_feat_dim; ++j) a += std::fabs((*pn.w0)[(size_t)n * pin + 12 + j]) * pl.B2[1 + j];
            Bp1[n] = a;
            m3n = std::max(m3n, a);
        }
        for (int n = 0; n < 64; ++n) {
            double a = std::fabs((*pn.c1)[n]);
            for (int k = 0; k < 64; ++k) a += std::fabs((*pn.w1)[(size_t)n * 64 + k]) * Bp1[k];
            m4n = std::max(m4n, a);
        }
    }
    for (int hid = 0; hid < 64; ++hid)
        for (int f = 0; f < 32; ++f) mwb = std::max(mwb, (double)std::fabs((*p.W1)[hid * 32 + f] * (*p.W2)[hid]));
    const bool finite_n = std::isfinite(m3n) && std::isfinite(m4n) && std::isfinite(mwb);
    const float s3n = finite_n && m3n > 0 ? pow2_floor(tgt / m3n) : 1.0f, s4n = finite_n && m4n > 0 ? pow2_floor(tgt / m4n) : 1.0f;
    const float gsc = finite_n && mwb > 0 ? pow2_floor(1024.0 / mwb) : 1.0f;
    out.grad_scale_normals = gsc;
    std::vector<float> P1n(P1.size(), 0.0f);
    for (int n = 0; n < 64; ++n) {
        for (int k = 0; k < sh; ++k) P1n[(size_t)n * cin_n + k] = (float)((double)P1[(size_t)n * cin_n + k] * s3n);
        for (int k = 0; k < d.geo_feat_dim; ++k) P1n[(size_t)n * cin_n + sh + k] = (float)((double)P1[(size_t)n * cin_n + sh + k] * ((double)s3n / pl.s2));
    }
    const std::vector<float> c0n = scaled(out.has_pred_normals ? *pn.c0 : z64, s3n);
    const std::vector<float> w1n = scaled(out.has_pred_normals ? *pn.w1 : z6464, (double)s4n / s3n), c1n = scaled(out.has_pred_normals ? *pn.c1 : z64, s4n);
    const std::vector<float> Wfn = scaled(Wf, 1.0 / s4n);
    std::vector<float> nimg_s = build_main_image(dn, W1s.data(), b1s.data(), W2s.data(), b2s.data(), P1n.data(), c0n.data(), w1n.data(), c1n.data(),
                                                 Wfn.data(), bf.data(), nullptr);
    nimg_s[SnMainImg::B3 + 3] = 1.0f / pl.s2;
    std::vector<float> wbs((size_t)64 * 32);
    for (int hid = 0; hid < 64; ++hid)
        for (int f = 0; f < 32; ++f) wbs[(size_t)hid * 32 + f] = (float)((double)((*p.W1)[hid * 32 + f] * (*p.W2)[hid]) * gsc);
    out.normals_split_ok = pl.ok && finite_n && fits_half(W1s) && fits_half(W2s) && fits_half(P1n) && fits_half(w1n) && fits_half(wbs);
    out.nh = build_main_image_h(dn, W1s.data(), W2s.data(), P1n.data(), w1n.data(), nimg_s);
    out.nh.resize(SnNormImgH::TOTAL_BYTES / 4, 0.0f);
    {
        uint16_t* hw = (uint16_t*)out.nh.data();
        for (int s4 = 0; s4 < 4; ++s4)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int f = lane & 31, hh = lane >> 5;
                    const int hid = (s4 / 2) * 32 + rho(8 * (s4 % 2) + e) + 4 * hh;
                    const float w = wbs[(size_t)hid * 32 + f];
                    const uint16_t hi = f32_to_f16_rne(w), lo = f32_to_f16_rne(w - f16_to_f32(hi));
                    const size_t off = (size_t)SnNormImgH::WB / 2 + ((size_t)(s4 * 2) * 64 + lane) * 8 + e;
                    hw[off] = hi;
                    hw[off + 512] = lo;
                }
    }
    return out;
}

// ---- proposal nets ------------------------------------------------------------------------------------------------------------
struct SnPropPack {
    std::vector<float> pack = std::vector<float>(SN_PROP_PACK_FLOATS, 0.0f);  // layout: sn_layout.h SN_PROP_*
    float t0p = 1.0f;  // the feature scale the net's de-hashed copies and paired tables carry
};

// w0 [16,10], b0 [16], w1 [16], b1 [1]
inline SnPropPack pack_proposal(const std::vector<float>& w0, const std::vector<float>& b0, const std::vector<float>& w1, const std::vector<float>& b1,
                                float table_absmax) {
    SnPropPack out;
    // range conditioning of the net's one matrix-core layer (see plan_split_scales): features carry t0p (stored in the net's
    // de-hashed copies and paired tables), the hidden layer s1p; both are divided out by the weights around them
    double t0p = 1.0, s1p = 1.0;
    if (std::isfinite(table_absmax) && table_absmax > 0.0f) {
        const double M = table_absmax;
        t0p = pow2_floor(1024.0 / M);
        double m1 = 0.0;
        for (int n = 0; n < 16; ++n) {
            double a = std::fabs(b0[n]);
            for (int k = 0; k < 10; ++k) a += std::fabs(w0[n * 10 + k]) * M;
            m1 = std::max(m1, a);
        }
        if (std::isfinite(m1) && m1 > 0.0) s1p = pow2_floor(16384.0 / m1);
        bool fits = true;
        for (int n = 0; n < 16; ++n) {
            fits = fits && std::fabs(b0[n] * s1p) <= 65504.0;
            for (int k = 0; k < 10; ++k) fits = fits && std::fabs(w0[n * 10 + k] * s1p / t0p) <= 65504.0;
        }
        if (!fits) t0p = s1p = 1.0;  // leave this net unconditioned (it only places samples)
    }
    out.t0p = (float)t0p;
    std::vector<float>& pack = out.pack;
    // W0 is stored k-major ([k][n]) so that two neighbouring hidden units share a register pair (v_pk_fma_f32)
    for (int n = 0; n < 16; ++n)
        for (int k = 0; k < 10; ++k) pack[SN_PROP_W0 + k * 16 + n] = (float)(w0[n * 10 + k] / t0p);
    memcpy(pack.data() + SN_PROP_B0, b0.data(), 16 * 4);
    memcpy(pack.data() + SN_PROP_W1, w1.data(), 16 * 4);
    pack[SN_PROP_B1] = b1[0];
    // matrix-core form (sn_prop_mlp_mfma): two A operands [lane][e], A[row = lane & 31][k = 8 (lane >> 5) + e], fp16 hi / lo
    // (lo = RNE(x - hi)).  Rows 0..15 are the hidden units for the rays of lanes 0..31 (k = 0..7), rows 16..31 the same units for
    // the rays of lanes 32..63 (k = 8..15); the other half of every row is zero.  Operand 1: e <-> W0[unit][e]; operand 2:
    // e = 0, 1 <-> W0[unit][8], W0[unit][9], e = 2 <-> b0[unit].
    {
        uint16_t* a1hi = (uint16_t*)(pack.data() + SN_PROP_MA1_HI);
        uint16_t* a1lo = (uint16_t*)(pack.data() + SN_PROP_MA1_LO);
        uint16_t* a2hi = (uint16_t*)(pack.data() + SN_PROP_MA2_HI);
        uint16_t* a2lo = (uint16_t*)(pack.data() + SN_PROP_MA2_LO);
        for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 8; ++e) {
                const int row = lane & 31, half = lane >> 5, unit = row & 15;
                float x1 = 0.0f, x2 = 0.0f;
                if ((row >> 4) == half) {
                    x1 = (float)(w0[unit * 10 + e] * s1p / t0p);
                    x2 = e < 2 ? (float)(w0[unit * 10 + 8 + e] * s1p / t0p) : (e == 2 ? (float)(b0[unit] * s1p) : 0.0f);
                }
                const uint16_t h1 = f32_to_f16_rne(x1), h2 = f32_to_f16_rne(x2);
                a1hi[lane * 8 + e] = h1;
                a1lo[lane * 8 + e] = f32_to_f16_rne(x1 - f16_to_f32(h1));
                a2hi[lane * 8 + e] = h2;
                a2lo[lane * 8 + e] = f32_to_f16_rne(x2 - f16_to_f32(h2));
            }
        // layer 2 as (w x + w |x|) / 2: MW1 holds w / 2 in accumulator order (per unit of the s1p-scaled accumulators), LIN the linear half
        for (int hh = 0; hh < 2; ++hh)
            for (int r = 0; r < 8; ++r) pack[SN_PROP_MW1 + hh * 8 + r] = (float)(0.5 * w1[(r & 3) + 8 * (r >> 2) + 4 * hh] / s1p);
        double cl = 0.0;
        for (int n = 0; n < 16; ++n) cl += (double)w1[n] * (double)b0[n];
        for (int k = 0; k < 10; ++k) {
            double v = 0.0;
            for (int n = 0; n < 16; ++n) v += (double)w1[n] * (double)w0[n * 10 + k];
            pack[SN_PROP_LIN + k] = (float)(0.5 * v / t0p);
        }
        pack[SN_PROP_LIN + 10] = (float)(0.5 * cl + (double)b1[0]);
    }
    return out;
}
