// wide_pack.cpp -- the host side of a wide main field (hidden_dim = hidden_dim_color = 128) as a stand-alone program
// (tests/test_wide_weights_host.py): signerf_amd/csrc/sn_weights.h (build_wide_image), sn_layout.h (SnWideImg) and sn_wide.h (the selector).
//
//   1. Packs seeded wide fields (appearance dims 0 / 32 / 128, both sh_remap values) and EMULATES the kernel's operand reads
//      (sn_wide_kernels.h sn_wide_layer / sn_wide_field_tile): for every layer, row tile, k-step and lane it reads the float the kernel
//      reads from the image as A[i][k], multiplies by seeded activations placed in the MFMA's B / D register layout
//      (v_mfma_f32_32x32x2_f32: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31], D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31])
//      and compares with a plain W . x + b in double.  One line per case: "pack ... max_rel_err <e> OK|FAIL".
//   2. Prints the selector's answer for every (grid, nprop, precision, spacing, box, dump, stats) on a wide handle.
// Exit status 0 when every case agrees within 1e-6 relative.
#include "../../signerf_amd/csrc/sn_weights.h"
#include "../../signerf_amd/csrc/sn_wide.h"

#include <cstdio>

static uint32_t g_state = 12345u;
static float rnd() {  // uniform in [-1, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (float)((double)(g_state >> 8) / 8388608.0 - 1.0);
}
static std::vector<float> rvec(size_t n, float gain) {
    std::vector<float> v(n);
    for (float& x : v) x = rnd() * gain;
    return v;
}

constexpr int H = SnWideImg::HIDDEN;
static int d_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }  // row of accumulator register r in lane half h

// The MFMA products of one layer as the kernel issues them (sn_wide_layer<RT, KS>): out[rt][r][lane] for 64 lanes, from the image and the B
// operand op[t][lane]; the bias image initialises the accumulators.
static void emulate_layer(const std::vector<float>& img, int wbase, int rt_stride, int bbase, int RT, int KS, const std::vector<double>& op /*[KS][64]*/,
                          std::vector<double>& acc /*[RT][16][64]*/) {
    acc.assign((size_t)RT * 16 * 64, 0.0);
    for (int rt = 0; rt < RT; ++rt)
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 16; ++r) acc[((size_t)rt * 16 + r) * 64 + lane] = img[bbase + (rt * 2 + (lane >> 5)) * 16 + r];
    for (int rt = 0; rt < RT; ++rt)
        for (int t = 0; t < KS; ++t) {
            // D[i][j] += sum over k = 0, 1 of A[i][k] B[k][j]; A[i][k] sits in lane 32 k + i, B[k][j] in lane 32 k + j
            for (int i = 0; i < 32; ++i)
                for (int j = 0; j < 32; ++j) {
                    double s = 0.0;
                    for (int k = 0; k < 2; ++k) {
                        const float a = img[wbase + rt * rt_stride + ((t / 4) * 64 + (32 * k + i)) * 4 + (t % 4)];  // the kernel's f32x4 read, element t % 4
                        s += (double)a * op[(size_t)t * 64 + 32 * k + j];
                    }
                    // D[i][j] lives in register r of lane 32 h + j with d_row(r, h) == i
                    for (int h = 0; h < 2; ++h)
                        for (int r = 0; r < 16; ++r)
                            if (d_row(r, h) == i) acc[((size_t)rt * 16 + r) * 64 + 32 * h + j] += s;
                }
        }
}

struct Worst {
    double err = 0.0;
    void see(double got, double want, double scale) { err = std::max(err, std::fabs(got - want) / scale); }
};

static double absmax(const std::vector<double>& v) {
    double m = 1e-30;
    for (double x : v) m = std::max(m, std::fabs(x));
    return m;
}

static bool pack_case(int app_dim, int sh_remap) {
    SnFieldDesc d{};
    d.geo_feat_dim = 15;
    d.sh_levels = 4;
    d.sh_remap = sh_remap;
    d.appearance_embed_dim = app_dim;
    d.hidden_dim_color = H;
    d.main_field.hidden_dim = H;
    const int sh = 16, geo = 15, cin = sh + geo + app_dim;
    const std::vector<float> W1 = rvec((size_t)H * 32, 0.4f), b1 = rvec(H, 0.3f), W2 = rvec((size_t)16 * H, 0.3f), b2 = rvec(16, 0.3f);
    const std::vector<float> Wc1 = rvec((size_t)H * cin, 0.3f), bc1 = rvec(H, 0.3f), Wc2 = rvec((size_t)H * H, 0.2f), bc2 = rvec(H, 0.3f);
    const std::vector<float> Wc3 = rvec((size_t)3 * H, 0.3f), bc3 = rvec(3, 0.3f), app = rvec((size_t)app_dim, 1.0f);
    const SnMainTensors mt{&W1, &b1, &W2, &b2, &Wc1, &bc1, &Wc2, &bc2, &Wc3, &bc3, &app};
    const std::vector<float> img = pack_wide_image(d, mt);
    if ((int)img.size() != SnWideImg::TOTAL || !sn_is_wide(d)) return false;
    Worst w;
    // seeded activations of the 32 samples of one tile, plain order: x[j][n]
    auto seeded = [&](int n) {
        std::vector<double> x((size_t)32 * n);
        for (double& v : x) v = rnd();
        return x;
    };
    // a 128-wide activation vector placed as the accumulators of the layer before hold it, read as the kernel's next operand:
    // op[t = rt 16 + r][lane = 32 h + j] = x[j][32 rt + d_row(r, h)]
    auto op_from_acc_layout = [&](const std::vector<double>& x, bool relu) {
        std::vector<double> op((size_t)64 * 64);
        for (int t = 0; t < 64; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const double v = x[(size_t)(lane & 31) * H + (t / 16) * 32 + d_row(t % 16, lane >> 5)];
                op[(size_t)t * 64 + lane] = relu ? std::max(v, 0.0) : v;
            }
        return op;
    };
    std::vector<double> acc;
    // ---- layer 1: op[t][32 h + j] = feature 2t + h of sample j (what sn_swap_halves leaves in a tile's operand) ----
    {
        const std::vector<double> x = seeded(32);
        std::vector<double> op((size_t)16 * 64);
        for (int t = 0; t < 16; ++t)
            for (int lane = 0; lane < 64; ++lane) op[(size_t)t * 64 + lane] = x[(size_t)(lane & 31) * 32 + 2 * t + (lane >> 5)];
        emulate_layer(img, SnWideImg::W1, 1024, SnWideImg::B1, 4, 16, op, acc);
        std::vector<double> want((size_t)32 * H);
        for (int j = 0; j < 32; ++j)
            for (int n = 0; n < H; ++n) {
                double s = b1[n];
                for (int k = 0; k < 32; ++k) s += (double)W1[n * 32 + k] * x[(size_t)j * 32 + k];
                want[(size_t)j * H + n] = s;
            }
        const double sc = absmax(want);
        for (int rt = 0; rt < 4; ++rt)
            for (int r = 0; r < 16; ++r)
                for (int lane = 0; lane < 64; ++lane)
                    w.see(acc[((size_t)rt * 16 + r) * 64 + lane], want[(size_t)(lane & 31) * H + rt * 32 + d_row(r, lane >> 5)], sc);
    }
    // ---- layer 2: 128 -> 32 padded rows (0..15 real, 20 = row 0 again, rest zero) ----
    std::vector<double> l2((size_t)32 * 16);  // plain layer-2 outputs of the 32 samples, reused as colour layer 1's inputs
    {
        const std::vector<double> x = seeded(H);
        emulate_layer(img, SnWideImg::W2, 0, SnWideImg::B2, 1, 64, op_from_acc_layout(x, true), acc);
        for (int j = 0; j < 32; ++j)
            for (int n = 0; n < 16; ++n) {
                double s = b2[n];
                for (int k = 0; k < H; ++k) s += (double)W2[n * H + k] * std::max(x[(size_t)j * H + k], 0.0);
                l2[(size_t)j * 16 + n] = s;
            }
        const double sc = absmax(l2);
        for (int r = 0; r < 16; ++r)
            for (int lane = 0; lane < 64; ++lane) {
                const int row = d_row(r, lane >> 5);
                const double want = row < 16 ? l2[(size_t)(lane & 31) * 16 + row] : (row == 20 ? l2[(size_t)(lane & 31) * 16] : 0.0);
                w.see(acc[(size_t)r * 64 + lane], want, sc);
            }
        // the upper half-wave finds its sample's h0 in register 8 (row 20)
        if (d_row(8, 1) != 20 || d_row(0, 0) != 0) return false;
    }
    // ---- colour layer 1: k-steps 0..7 = layer-2 registers 0..7 (rows d_row(t, h)), 8..15 = SH component 2 (t - 8) + h; appearance in the bias ----
    {
        const std::vector<double> shv = seeded(16);
        std::vector<double> op((size_t)16 * 64);
        for (int t = 0; t < 16; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const int j = lane & 31, h = lane >> 5;
                op[(size_t)t * 64 + lane] = t < 8 ? l2[(size_t)j * 16 + d_row(t, h)] : shv[(size_t)j * 16 + 2 * (t - 8) + h];
            }
        emulate_layer(img, SnWideImg::WC1, 1024, SnWideImg::BC1, 4, 16, op, acc);
        std::vector<double> want((size_t)32 * H);
        for (int j = 0; j < 32; ++j)
            for (int n = 0; n < H; ++n) {
                double s = bc1[n];
                for (int k = 0; k < sh; ++k) s += (double)Wc1[(size_t)n * cin + k] * shv[(size_t)j * 16 + k];
                for (int k = 0; k < geo; ++k) s += (double)Wc1[(size_t)n * cin + sh + k] * l2[(size_t)j * 16 + 1 + k];
                for (int k = 0; k < app_dim; ++k) s += (double)Wc1[(size_t)n * cin + sh + geo + k] * (double)app[k];
                want[(size_t)j * H + n] = s;
            }
        const double sc = absmax(want);
        for (int rt = 0; rt < 4; ++rt)
            for (int r = 0; r < 16; ++r)
                for (int lane = 0; lane < 64; ++lane)
                    w.see(acc[((size_t)rt * 16 + r) * 64 + lane], want[(size_t)(lane & 31) * H + rt * 32 + d_row(r, lane >> 5)], sc);
    }
    // ---- colour layer 2 (two passes of two row tiles, as the kernel runs it) and colour layer 3 on the VALU ----
    {
        const std::vector<double> x = seeded(H);
        const std::vector<double> op = op_from_acc_layout(x, true);
        std::vector<double> want((size_t)32 * H), rgbw((size_t)32 * 3), part((size_t)3 * 64, 0.0);
        for (int j = 0; j < 32; ++j) {
            for (int n = 0; n < H; ++n) {
                double s = bc2[n];
                for (int k = 0; k < H; ++k) s += (double)Wc2[n * H + k] * std::max(x[(size_t)j * H + k], 0.0);
                want[(size_t)j * H + n] = s;
            }
            for (int c = 0; c < 3; ++c) {
                double s = bc3[c];
                for (int n = 0; n < H; ++n) s += (double)Wc3[c * H + n] * std::max(want[(size_t)j * H + n], 0.0);
                rgbw[(size_t)j * 3 + c] = s;
            }
        }
        const double sc = absmax(want), sc3 = absmax(rgbw);
        for (int pass = 0; pass < 2; ++pass) {
            emulate_layer(img, SnWideImg::WC2 + pass * 2 * 4096, 4096, SnWideImg::BC2 + pass * 64, 2, 64, op, acc);
            for (int rtl = 0; rtl < 2; ++rtl)
                for (int r = 0; r < 16; ++r)
                    for (int lane = 0; lane < 64; ++lane) {
                        const double got = acc[((size_t)rtl * 16 + r) * 64 + lane];
                        w.see(got, want[(size_t)(lane & 31) * H + (pass * 2 + rtl) * 32 + d_row(r, lane >> 5)], sc);
                        for (int c = 0; c < 3; ++c)  // the kernel's x[j = rtl 16 + r] against W3[(c 2 + h) 64 + pass 32 + j]
                            part[(size_t)c * 64 + lane] += (double)img[SnWideImg::W3 + (c * 2 + (lane >> 5)) * 64 + pass * 32 + rtl * 16 + r] * std::max(got, 0.0);
                    }
        }
        for (int j = 0; j < 32; ++j)
            for (int c = 0; c < 3; ++c)  // the two half-wave partial sums of a sample + the bias
                w.see(part[(size_t)c * 64 + j] + part[(size_t)c * 64 + 32 + j] + img[SnWideImg::B3 + c], rgbw[(size_t)j * 3 + c], sc3);
    }
    const bool ok = w.err <= 1e-6;
    printf("pack app %d sh_remap %d image_floats %d max_rel_err %.3e %s\n", app_dim, sh_remap, (int)img.size(), w.err, ok ? "OK" : "FAIL");
    return ok;
}

static void print_selector() {
    for (int grid = 0; grid < 2; ++grid)
        for (int nprop = 0; nprop <= 2; ++nprop)
            for (int prec = 0; prec <= 2; ++prec)
                for (int spacing = 0; spacing < 2; ++spacing)
                    for (int box = 0; box < 2; ++box)
                        for (int dump = 0; dump < 2; ++dump)
                            for (int stats = 0; stats < 2; ++stats) {
                                SnVariantFacts f{};
                                f.main_grid_mode = f.prop_grid_mode = grid;
                                f.nd_prop[0] = 5;
                                f.nd_prop[1] = 4;
                                f.td_prop[0] = f.td_prop[1] = grid ? 3 : 0;
                                f.box = box;
                                f.num_proposals = 2;
                                SnVariantRequest r{};
                                r.num_proposal_iterations = nprop;
                                r.precision = prec;
                                r.spacing_mode = spacing;
                                r.far_plane = 1000.0f;
                                r.dump = dump != 0;
                                r.march_stats = stats != 0;
                                const SnWideMainSelection s = sn_select_main_wide(f, r);
                                printf("select grid %d nprop %d prec %d spacing %d box %d dump %d stats %d -> ", grid, nprop, prec, spacing, box, dump, stats);
                                if (s.err) printf("refused %d: %s\n", s.err, s.text);
                                else printf("sn_wide_field_main_kernel<%d, %d> effective_precision %d\n", s.v.mode, s.v.grid, sn_effective_precision_wide(f, prec, 0));
                            }
    SnRenderOpts o{};
    o.num_nerf_samples = 128;
    o.chunk_rays = 32768;
    const SnFramePlan plan = sn_plan_frame(100, 100, o, 256);
    const SnWideLaunch l0 = sn_wide_main_launch(plan, 0), l2 = sn_wide_main_launch(plan, 2);
    printf("launch 100x100x128 grid %u lds_bytes %zu (bins %zu) / with proposals %zu; limit %zu\n", l0.grid, l0.lds_bytes, l0.etab_bytes, l2.lds_bytes,
           kSnWideMaxLdsBytes);
    printf("widths (64,64) %d (128,128) %d (32,32) %d (128,64) %d (64,128) %d\n", sn_width_pair_supported(64, 64), sn_width_pair_supported(128, 128),
           sn_width_pair_supported(32, 32), sn_width_pair_supported(128, 64), sn_width_pair_supported(64, 128));
}

int main() {
    bool ok = true;
    const int apps[3] = {0, 32, 128};
    for (int a : apps)
        for (int remap = 0; remap < 2; ++remap) ok = pack_case(a, remap) && ok;
    print_selector();
    return ok ? 0 : 1;
}
