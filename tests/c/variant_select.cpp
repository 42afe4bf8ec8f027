// variant_select.cpp -- the launch selectors of signerf_amd/csrc/sn_variant.h as a stand-alone program (tests/test_variant_select_host.py,
// tests/test_launch_variants_host.py).
//
//     variant_select lists        the mangled name of every instantiation the three lists build, one per line
//     variant_select enumerate    the product of facts x requests: every selection is in its list, every refusal has a code and a text;
//                                 prints the counts and the listed instantiations no combination selected
//     variant_select check FILE   recorded calls, one per line, tab separated:
//                                     numbers <TAB> K1 name or - <TAB> K2 name or - <TAB> normals name or - <TAB> refusal text or empty
//                                 numbers = main grid_mode, proposal grid_mode, log2_hashmap_size, num_proposals, nd_torch, nd_prop[2], split_ok,
//                                 normals_split_ok, has_half_grid, has_dense_main, box, 16 main scalings, 2 x 5 proposal scalings, then the call:
//                                 entry (0 sn_render_rays, 1 sn_render_rays_debug, 2 sn_render_normals), num_proposal_iterations, precision,
//                                 spacing_mode, far_plane, march_stats, reuse_final_bins
// Exit status 0 when every check held; failures go to stderr.
#include "../../signerf_amd/csrc/sn_variant.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

static std::string arg(int v) { return v < 0 ? "Lin" + std::to_string(-v) + "E" : "Li" + std::to_string(v) + "E"; }
static std::string flag(int v) { return v ? "Lb1E" : "Lb0E"; }
static std::string name(const SnMainVariant& v) {
    return "_Z21sn_render_main_kernelI" + arg(v.mode) + arg(v.prec) + arg(v.grid) + arg(v.nd) + flag(v.dump) + flag(v.alt) + flag(v.stats) + "Ev12SnMainParams";
}
static std::string name(const SnPropVariant& v) {
    return "_Z18sn_proposal_kernelI" + arg(v.grid) + arg(v.nd0) + arg(v.nd1) + flag(v.dump) + flag(v.alt) + flag(v.stats) + "Ev12SnPropParams";
}
static std::string name(const SnNormalsVariant& v) {
    return "_Z17sn_normals_kernelI" + arg(v.mode) + arg(v.grid) + arg(v.prec) + arg(v.nd) + flag(v.alt) + "Ev15SnNormalsParams";
}

#define X(...) SnMainVariant{__VA_ARGS__},
static const std::vector<SnMainVariant> kMain = {SN_MAIN_VARIANTS(X)};
#undef X
#define X(...) SnPropVariant{__VA_ARGS__},
static const std::vector<SnPropVariant> kProp = {SN_PROP_VARIANTS(X)};
#undef X
#define X(...) SnNormalsVariant{__VA_ARGS__},
static const std::vector<SnNormalsVariant> kNormals = {SN_NORMALS_VARIANTS(X)};
#undef X

static int g_failures = 0;
static void failed(const std::string& what) {
    if (++g_failures <= 20) fprintf(stderr, "variant_select: %s\n", what.c_str());
}

template <typename V>
static int index_of(const std::vector<V>& list, const V& v) {
    for (size_t i = 0; i < list.size(); ++i)
        if (sn_same_variant(list[i], v)) return (int)i;
    return -1;
}

// one selection against its list; `used` counts what was selected
template <typename SEL, typename V>
static void audit(const SEL& s, const std::vector<V>& list, std::vector<long>& used, const char* which) {
    if (s.err) {
        if (s.err != SN_ERR_INVALID || !s.text || !*s.text) failed(std::string(which) + ": a refusal without code or text");
        return;
    }
    const int i = index_of(list, s.v);
    if (i < 0) failed(std::string(which) + ": selected " + name(s.v) + ", which is not built");
    else ++used[(size_t)i];
}

static int enumerate() {
    std::vector<long> used_main(kMain.size(), 0), used_prop(kProp.size(), 0), used_normals(kNormals.size(), 0);
    const int nd_torch[] = {0, kSnBcMain, kSnDenseLevelsDefault, 5}, td_main[] = {-1, 0, 12};
    const int prop[][4] = {{5, 4, 0, 0}, {5, 4, -1, 0}, {5, 4, 3, 5}, {5, 5, 0, 0}, {0, 0, 0, 0}};  // nd_prop[2], td_prop[2]
    const float far_plane[] = {1000.0f, 2.0e7f, std::nanf("")};
    long combos = 0, refused = 0, invalid = 0;
    for (int bits = 0; bits < 128; ++bits)
        for (int ndt : nd_torch) for (int tdm : td_main) for (auto& pr : prop) for (int nets = 0; nets <= SN_MAX_PROPOSALS; ++nets) {
            SnVariantFacts f{};
            f.main_grid_mode = bits & 1, f.prop_grid_mode = (bits >> 1) & 1;
            f.split_ok = bits & 4, f.normals_split_ok = bits & 8, f.has_half_grid = bits & 16, f.has_dense_main = bits & 32, f.box = (bits >> 6) & 1;
            f.nd_torch = ndt, f.td_main = tdm, f.num_proposals = nets;
            for (int i = 0; i < SN_MAX_PROPOSALS; ++i) f.nd_prop[i] = pr[i], f.td_prop[i] = pr[2 + i];
            SnFieldDesc d{};
            d.main_field.grid_mode = f.main_grid_mode, d.num_proposals = nets;
            for (int nprop = 0; nprop <= nets + 1 && nprop <= SN_MAX_PROPOSALS; ++nprop) for (int prec = 0; prec <= 2; ++prec) for (int spacing = 0; spacing <= 1; ++spacing)
                for (float fp : far_plane) for (int flags = 0; flags < 4; ++flags) {
                    const SnVariantRequest r{nprop, prec, spacing, fp, (flags & 1) != 0, (flags & 2) != 0};
                    SnRenderOpts o{};
                    o.num_proposal_iterations = nprop, o.num_nerf_samples = 48, o.chunk_rays = 1, o.precision = prec, o.spacing_mode = spacing;
                    o.num_proposal_samples[0] = o.num_proposal_samples[1] = 8;
                    std::string why;
                    ++combos;
                    if (!valid_opts(d, o, why)) {    // the entry points stop here: the selectors never see such a request
                        if (why.empty()) failed("valid_opts refused without a text");
                        ++invalid;
                        continue;
                    }
                    const SnMainSelection m = sn_select_main(f, r);
                    const SnNormalsSelection n = sn_select_normals(f, r);
                    audit(m, kMain, used_main, "sn_select_main");
                    audit(n, kNormals, used_normals, "sn_select_normals");
                    refused += m.err != 0;
                    if (nprop > 0) {
                        const SnPropSelection p = sn_select_proposal(f, r);
                        audit(p, kProp, used_prop, "sn_select_proposal");
                        if (p.err && !m.err) failed("a colour render was selected whose proposal kernel is refused");
                    }
                    if (!m.err && (m.v.prec != sn_effective_precision_of(f, prec, 0) || n.v.prec != sn_effective_precision_of(f, prec, 1)))
                        failed("sn_effective_precision_of disagrees with the selected precision");
                }
        }
    printf("combinations %ld invalid %ld refused %ld\n", combos, invalid, refused);
    for (size_t i = 0; i < kMain.size(); ++i) if (!used_main[i]) printf("never selected %s\n", name(kMain[i]).c_str());
    for (size_t i = 0; i < kProp.size(); ++i) if (!used_prop[i]) printf("never selected %s\n", name(kProp[i]).c_str());
    for (size_t i = 0; i < kNormals.size(); ++i) if (!used_normals[i]) printf("never selected %s\n", name(kNormals[i]).c_str());
    return g_failures ? 1 : 0;
}

static int check(const char* path) {
    std::ifstream in(path);
    std::string line;
    long n_lines = 0;
    while (std::getline(in, line)) {
        std::vector<std::string> col;
        std::stringstream cols(line);
        for (std::string c; std::getline(cols, c, '\t');) col.push_back(c);
        col.resize(5);
        std::stringstream num(col[0]);
        SnHashMlpDesc grid[1 + SN_MAX_PROPOSALS] = {};
        SnVariantFacts f{};
        int log2_t = 0, split_ok = 0, normals_split_ok = 0, half = 0, dense = 0, entry = 0, march = 0, reuse = 0;
        num >> f.main_grid_mode >> f.prop_grid_mode >> log2_t >> f.num_proposals >> f.nd_torch >> f.nd_prop[0] >> f.nd_prop[1] >> split_ok >> normals_split_ok >>
            half >> dense >> f.box;
        f.split_ok = split_ok, f.normals_split_ok = normals_split_ok, f.has_half_grid = half, f.has_dense_main = dense;
        for (int g = 0; g < 1 + SN_MAX_PROPOSALS; ++g) {
            grid[g].num_levels = g ? 5 : 16, grid[g].log2_hashmap_size = log2_t, grid[g].grid_mode = g ? f.prop_grid_mode : f.main_grid_mode;
            for (int l = 0; l < grid[g].num_levels; ++l) num >> grid[g].scalings[l];
        }
        f.td_main = leading_dense(grid[0]);
        for (int i = 0; i < f.num_proposals; ++i) f.td_prop[i] = leading_dense(grid[1 + i]);
        SnVariantRequest r{};
        std::string far_text;
        num >> entry >> r.num_proposal_iterations >> r.precision >> r.spacing_mode >> far_text >> march >> reuse;
        if (!num) {
            failed("cannot parse line " + std::to_string(n_lines + 1));
            continue;
        }
        r.far_plane = strtof(far_text.c_str(), nullptr);
        r.dump = entry == 1, r.march_stats = march != 0;
        ++n_lines;
        std::string k1 = "-", k2 = "-", k3 = "-", text;
        const bool own_bins = r.num_proposal_iterations > 0 && !(entry == 2 && reuse);
        const SnPropSelection p = own_bins ? sn_select_proposal(f, r) : SnPropSelection{};
        if (entry == 2) {
            if (p.err) text = p.text;
            else k3 = name(sn_select_normals(f, r).v);
        } else {
            const SnMainSelection m = sn_select_main(f, r);
            if (m.err) text = m.text;
            else k1 = name(m.v);
        }
        if (text.empty() && own_bins) k2 = name(p.v);
        if (text != col[4]) failed("line " + std::to_string(n_lines) + ": refusal '" + text + "', recorded '" + col[4] + "'");
        else if (text.empty() && (k1 != col[1] || k2 != col[2] || k3 != col[3]))
            failed("line " + std::to_string(n_lines) + ": selected " + k1 + " " + k2 + " " + k3 + ", recorded " + col[1] + " " + col[2] + " " + col[3]);
    }
    printf("checked %ld\n", n_lines);
    return g_failures || n_lines == 0 ? 1 : 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "lists") {
        for (const auto& v : kMain) puts(name(v).c_str());
        for (const auto& v : kProp) puts(name(v).c_str());
        for (const auto& v : kNormals) puts(name(v).c_str());
        return 0;
    }
    if (mode == "enumerate") return enumerate();
    if (mode == "check" && argc > 2) return check(argv[2]);
    fprintf(stderr, "usage: variant_select lists | enumerate | check FILE\n");
    return 2;
}
