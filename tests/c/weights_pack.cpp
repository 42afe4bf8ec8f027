// weights_pack.cpp -- the host packers of signerf_amd/csrc/sn_weights.h as a stand-alone program (tests/test_weights_host.py).
//
//     weights_pack <input file> <output directory>
//
// Input, float32 little-endian (tests/weights_cases.py writes it): a header of 8 values
//     appearance_embed_dim, has_pred_normals, num_proposals, geo_feat_dim, sh_levels, abs-max of the main table, of proposal table 0, of table 1
// then the tensors, row-major: W1 [64,32], b1 [64], W2 [16,64], b2 [16], Wc1 [64,cin], bc1 [64], Wc2 [64,64], bc2 [64], Wc3 [3,64], bc3 [3]
// (cin = sh_levels^2 + geo_feat_dim + appearance_embed_dim); the mean appearance embedding [appearance_embed_dim] if that is > 0; if
// has_pred_normals: w0 [64,12+geo_feat_dim], c0 [64], w1 [64,64], c1 [64], w2 [64,64], c2 [64], head weight [3,64], head bias [3]; per
// proposal net: w0 [16,10], b0 [16], w1 [16], b1 [1].
// Output: main.bin, main_h.bin, normals.bin, normals_h.bin, prop<i>.bin -- the bytes sn_finalize_weights uploads -- and one JSON line
// of the scalars the handle keeps on stdout.
#include "../../signerf_amd/csrc/sn_weights.h"

#include <cstdio>

static std::vector<float> g_in;
static size_t g_pos = 0;

static std::vector<float> take(size_t n) {
    if (g_pos + n > g_in.size()) {
        fprintf(stderr, "weights_pack: input too short (%zu floats, need %zu)\n", g_in.size(), g_pos + n);
        exit(2);
    }
    std::vector<float> v(g_in.begin() + (long)g_pos, g_in.begin() + (long)(g_pos + n));
    g_pos += n;
    return v;
}

static void write_image(const std::string& dir, const std::string& name, const std::vector<float>& v) {
    const std::string path = dir + "/" + name + ".bin";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(v.data(), 4, v.size(), f) != v.size() || fclose(f) != 0) {
        fprintf(stderr, "weights_pack: cannot write %s\n", path.c_str());
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: weights_pack <input file> <output directory>\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "weights_pack: cannot read %s\n", argv[1]);
        return 2;
    }
    float buf[4096];
    for (size_t n; (n = fread(buf, 4, 4096, f)) > 0;) g_in.insert(g_in.end(), buf, buf + n);
    fclose(f);

    const std::vector<float> head = take(8);
    SnFieldDesc d;
    memset(&d, 0, sizeof(d));
    d.struct_size = sizeof(d);
    d.appearance_embed_dim = (int)head[0];
    const bool pred_normals = head[1] != 0.0f;
    d.num_proposals = (int)head[2];
    d.geo_feat_dim = (int)head[3];
    d.sh_levels = (int)head[4];
    if (d.appearance_embed_dim < 0 || d.appearance_embed_dim > 256 || d.num_proposals < 0 || d.num_proposals > SN_MAX_PROPOSALS ||
        d.geo_feat_dim != 15 || d.sh_levels != 4) {
        fprintf(stderr, "weights_pack: a header sn_create would refuse\n");
        return 2;
    }
    const size_t cin = (size_t)(d.sh_levels * d.sh_levels + d.geo_feat_dim + d.appearance_embed_dim), pin = 12 + (size_t)d.geo_feat_dim;

    const std::vector<float> W1 = take(64 * 32), b1 = take(64), W2 = take(16 * 64), b2 = take(16), Wc1 = take(64 * cin), bc1 = take(64),
                             Wc2 = take(64 * 64), bc2 = take(64), Wc3 = take(3 * 64), bc3 = take(3), app = take((size_t)d.appearance_embed_dim);
    const SnMainTensors mt{&W1, &b1, &W2, &b2, &Wc1, &bc1, &Wc2, &bc2, &Wc3, &bc3, &app};
    std::vector<float> pn[8];
    SnPredNormalTensors nt;
    if (pred_normals) {
        const size_t counts[8] = {64 * pin, 64, 64 * 64, 64, 64 * 64, 64, 3 * 64, 3};
        for (int i = 0; i < 8; ++i) pn[i] = take(counts[i]);
        nt.w0 = &pn[0], nt.c0 = &pn[1], nt.w1 = &pn[2], nt.c1 = &pn[3], nt.w2 = &pn[4], nt.c2 = &pn[5], nt.wh = &pn[6], nt.ch = &pn[7];
    }

    const std::string dir = argv[2];
    const SnMainImages main_img = pack_main_images(d, mt, head[5]);
    const SnNormalImages norm = pack_normal_images(d, mt, main_img, nt);
    write_image(dir, "main", main_img.img);
    write_image(dir, "main_h", main_img.imgh);
    write_image(dir, "normals", norm.nimg);
    write_image(dir, "normals_h", norm.nh);
    float t0p[SN_MAX_PROPOSALS] = {0.0f, 0.0f};
    for (int i = 0; i < d.num_proposals; ++i) {
        const std::vector<float> w0 = take(16 * 10), b0 = take(16), w1 = take(16), pb1 = take(1);
        const SnPropPack pp = pack_proposal(w0, b0, w1, pb1, head[6 + i]);
        write_image(dir, "prop" + std::to_string(i), pp.pack);
        t0p[i] = pp.t0p;
    }
    if (g_pos != g_in.size()) {
        fprintf(stderr, "weights_pack: %zu floats of input left over\n", g_in.size() - g_pos);
        return 2;
    }
    const MainSplitPlan& pl = main_img.plan;
    printf("{\"t0\": %.17g, \"s1\": %.17g, \"s2\": %.17g, \"s3\": %.17g, \"s4\": %.17g, \"split_ok\": %d, \"normals_split_ok\": %d, "
           "\"has_pred_normals\": %d, \"grad_scale_normals\": %.17g, \"t0p\": [",
           pl.t0, pl.s1, pl.s2, pl.s3, pl.s4, (int)main_img.split_ok, (int)norm.normals_split_ok, (int)norm.has_pred_normals, norm.grad_scale_normals);
    for (int i = 0; i < d.num_proposals; ++i) printf("%s%.17g", i ? ", " : "", t0p[i]);
    printf("], \"split_why\": \"%s\", \"sizes\": {\"main\": %zu, \"main_h\": %zu, \"normals\": %zu, \"normals_h\": %zu, \"prop\": %zu}}\n",
           main_img.split_why.c_str(), main_img.img.size() * 4, main_img.imgh.size() * 4, norm.nimg.size() * 4, norm.nh.size() * 4,
           (size_t)SN_PROP_PACK_FLOATS * 4);
    return 0;
}
