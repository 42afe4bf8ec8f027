// sn_variant.h -- which instantiation of the three fused kernels a call launches: sn_render_main_kernel (K1, sn_main.h),
// sn_proposal_kernel (K2, sn_proposal.h) and sn_normals_kernel (sn_normals.h).  Plain C++17, no HIP: tests/c/variant_select.cpp compiles
// this header alone and enumerates it, and tests/test_launch_variants_host.py holds what sn_api.hip launches with it against the launches
// recorded from the commit that still decided inside the launch sites (tests/golden/launch_variants.json).
//   * SnVariantFacts / SnVariantRequest: what selection depends on -- a finalized handle's side, a call's side;
//   * sn_select_main / sn_select_proposal / sn_select_normals: the template arguments, the flags the launcher fills its parameters from,
//     or a refusal (every one is SN_ERR_INVALID with a fixed text);
//   * SN_MAIN_VARIANTS / SN_PROP_VARIANTS / SN_NORMALS_VARIANTS: every tuple that is built.  sn_api.hip generates its tables of kernel
//     pointers from them; a selection that is in no list is a bug and is reported as one, never replaced by another kernel.
#pragma once
#include "../../include/signerf_hip.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

constexpr int kSnDenseLevelsDefault = 11;  // the copy counts sn_finalize_weights leaves a main grid with: this, kSnBcMain or none
constexpr int kSnBcMain = 9;
constexpr int kSnPropMaxSamples = 256;     // (sn_api.hip asserts that these three are the kernels' SN_DENSE_LEVELS_DEFAULT, SN_BC_MAIN, SN_PROP_MAX_SAMPLES)

// tiny-cuda-nn level table (grid_mode 1): resolution = ceil(scale) + 1; a level is indexed densely when its whole grid fits the table.
// Returns that resolution, or 0 for a hashed level and for every level of a torch grid.
inline uint32_t sn_tcnn_dense_res(const SnHashMlpDesc& d, int l) {
    if (d.grid_mode != 1) return 0;
    const uint64_t T = 1ull << d.log2_hashmap_size;
    const uint64_t res = (uint64_t)ceilf(d.scalings[l]) + 1;
    return res * res * res <= T && res <= 255 ? (uint32_t)res : 0u;
}

// number of leading dense levels if the dense levels form a prefix of the level list, else -1 (0 for a torch grid)
inline int leading_dense(const SnHashMlpDesc& d) {
    int nd = 0;
    bool ended = false;
    for (int l = 0; l < d.num_levels; ++l) {
        const bool dense = sn_tcnn_dense_res(d, l) != 0u;
        if (dense && ended) return -1;
        if (dense) ++nd;
        else ended = true;
    }
    return nd;
}

struct SnVariantFacts {
    int main_grid_mode, prop_grid_mode;  // SnHashMlpDesc.grid_mode of the main field / of proposal net 0 (0 torch, 1 tiny-cuda-nn)
    int nd_torch;                        // de-hashed copies of the main grid (0, kSnBcMain or kSnDenseLevelsDefault)
    int nd_prop[SN_MAX_PROPOSALS];       // ... of the proposal nets
    int td_main, td_prop[SN_MAX_PROPOSALS];  // leading_dense of the same grids
    bool split_ok, normals_split_ok;     // the range-conditioned fp16 operands exist (sn_weights.h plan_split_scales)
    bool has_half_grid;                  // SnFieldDesc.half_grid: both fp16 buffers of the main grid were built
    bool has_dense_main;                 // the buffer of the main grid's de-hashed copies
    int box;                             // SnPosMap.box = SnFieldDesc.disable_scene_contraction
    int num_proposals;
};

struct SnVariantRequest {
    int num_proposal_iterations, precision, spacing_mode;
    float far_plane;
    bool dump;         // sn_render_rays_debug
    bool march_stats;  // SnRenderOpts.march_stats is set
};

inline bool sn_precision_supported(int main_grid_mode, int precision) {
    return precision >= 0 && precision <= 2 && (precision != 2 || main_grid_mode == 1);  // single fp16 is the arithmetic of tiny-cuda-nn checkpoints
}

inline bool valid_opts(const SnFieldDesc& d, const SnRenderOpts& o, std::string& why) {
    if (o.num_proposal_iterations < 0 || o.num_proposal_iterations > d.num_proposals) why = "num_proposal_iterations exceeds the proposal nets of this handle";
    else if (o.num_nerf_samples < 1 || o.num_nerf_samples > 1024) why = "num_nerf_samples out of range [1,1024]";
    else if (o.chunk_rays < 1) why = "chunk_rays must be positive";
    else if (o.precision < 0 || o.precision > 2) why = "precision must be 0 (fp32), 1 (split fp16) or 2 (single fp16, tiny-cuda-nn grids)";
    else if (!sn_precision_supported(d.main_field.grid_mode, o.precision))
        why = "precision 2 (single fp16) is the arithmetic of tiny-cuda-nn checkpoints: it needs main_field.grid_mode = 1";
    else if (o.background_mode != 0 && o.background_mode != 1) why = "background_mode must be 0 (last sample) or 1 (constant colour)";
    else if (o.spacing_mode != 0 && o.spacing_mode != 1) why = "spacing_mode must be 0 (piecewise) or 1 (uniform)";
    else {
        for (int i = 0; i < o.num_proposal_iterations; ++i)
            if (o.num_proposal_samples[i] < 2 || o.num_proposal_samples[i] > kSnPropMaxSamples) {
                why = "num_proposal_samples out of range [2," + std::to_string(kSnPropMaxSamples) + "]";
                return false;
            }
        return true;
    }
    return false;
}

// The non-default sampler / position map run in the ALT instantiations of all three kernels (run-time-generic: uploaded tables, no de-hashed
// copies, STRICT position arithmetic), so that the production kernels' code does not depend on them.  A far plane beyond 1e7 goes there
// too: out there the exact contraction rounds onto the face q = 1 (dropped by the selector) and the production kernels' reciprocal
// form may not (sn_sample_q_fast).
inline bool needs_generic_kernels(const SnVariantFacts& f, const SnVariantRequest& r) {
    return r.spacing_mode != 0 || f.box != 0 || !(r.far_plane <= 1.0e7f);
}

// what a precision request resolves to: a handle whose weights cannot be range-conditioned renders in exact fp32; the normals kernel
// keeps the split form under a single-fp16 request
inline int sn_main_precision(const SnVariantFacts& f, int requested) { return requested >= 1 && f.split_ok ? requested : 0; }
inline int sn_normals_precision(const SnVariantFacts& f, int requested) { return requested >= 1 && f.normals_split_ok ? 1 : 0; }
inline int sn_effective_precision_of(const SnVariantFacts& f, int requested, int kernel) {  // kernel 0: render / field kernels, 1: normals
    if ((kernel != 0 && kernel != 1) || !sn_precision_supported(f.main_grid_mode, requested)) return -1;
    return kernel == 0 ? sn_main_precision(f, requested) : sn_normals_precision(f, requested);
}

// The template arguments of the three kernels, in the kernels' order (all int, so that two tuples compare as bytes)
struct SnMainVariant { int mode, prec, grid, nd, dump, alt, stats; };
struct SnPropVariant { int grid, nd0, nd1, dump, alt, stats; };
struct SnNormalsVariant { int mode, grid, prec, nd, alt; };
template <typename V>
bool sn_same_variant(const V& a, const V& b) { return memcmp(&a, &b, sizeof(V)) == 0; }

template <typename V>
struct SnSelection {
    int err;             // SN_OK, or the refusal's code with its text
    const char* text;
    V v;
    // what the launcher fills its parameters from
    bool split, half1;   // the fp16 weight image; K1: single fp16 (its own LDS image, no tail split)
    bool copies;         // grid / dense = the de-hashed copies (else the tiny-cuda-nn level table of the uploaded grid)
    bool hgrid;          // K1, single fp16: the grid is read from its fp16 storage
};
using SnMainSelection = SnSelection<SnMainVariant>;
using SnPropSelection = SnSelection<SnPropVariant>;
using SnNormalsSelection = SnSelection<SnNormalsVariant>;
template <typename V>
SnSelection<V> sn_refuse(const char* text) { return SnSelection<V>{SN_ERR_INVALID, text, {}, false, false, false, false}; }

inline SnPropSelection sn_select_proposal(const SnVariantFacts& f, const SnVariantRequest& r) {
    auto refuse = sn_refuse<SnPropVariant>;
    auto take = [](int grid, int nd0, int nd1, bool dump, bool alt, bool stats) {
        return SnPropSelection{SN_OK, "", {grid, nd0, nd1, dump, alt, stats}, false, false, nd0 >= 0, false};
    };
    const bool alt = needs_generic_kernels(f, r), tcnn = f.prop_grid_mode == 1;
    // nerfacto's proposal nets (max_res 128 / 256): 5 and 4 levels have de-hashed copies -- every level but the finest of the second net
    const bool def = r.num_proposal_iterations == 2 && f.nd_prop[0] == 5 && f.nd_prop[1] == 4;
    if (r.dump && alt) return refuse("sn_render_rays_debug: the dump exists for the default sampler and scene contraction only");
    if (r.march_stats && (r.dump || alt || tcnn || !def))
        return refuse("SnRenderOpts.march_stats: the counting instantiation of the proposal kernel exists for the default variant only (torch grid, 2 nets, 5 + 4 de-hashed levels, default sampler)");
    if (alt) return take(tcnn, -1, -1, false, true, false);
    if (r.dump) {  // the instrumented instantiation exists for the production variant of nerfacto's proposal nets only
        if (tcnn || !def)
            return refuse("sn_render_rays_debug: the proposal-kernel dump exists for the default variant only (torch grid, 2 nets, 5 + 4 de-hashed levels)");
        return take(0, 5, 4, true, false, false);
    }
    // tiny-cuda-nn: the copies must cover every level it indexes densely (3 and 2 at T = 2^17); other shapes read the uploaded tables
    // with the per-level run-time decision
    if (tcnn) return def && f.td_prop[0] >= 0 && f.td_prop[0] <= 5 && f.td_prop[1] >= 0 && f.td_prop[1] <= 4 ? take(1, 5, 4, false, false, false)
                                                                                                         : take(1, -1, -1, false, false, false);
    return def ? take(0, 5, 4, false, false, r.march_stats) : take(0, -1, -1, false, false, false);
}

// Every refusal of a colour render, in the order a call meets them: the counting instantiations, the proposal kernel's (a render with
// proposal iterations launches it first), then the single-fp16 and instrumented ones of K1.
inline SnMainSelection sn_select_main(const SnVariantFacts& f, const SnVariantRequest& r) {
    auto refuse = sn_refuse<SnMainVariant>;
    const bool alt = needs_generic_kernels(f, r), tcnn = f.main_grid_mode == 1;
    const int prec = sn_main_precision(f, r.precision), mode = r.num_proposal_iterations > 0;
    const bool split = prec >= 1, half1 = prec == 2;
    // de-hashed copies are used when they cover every level tiny-cuda-nn indexes densely (always true for torch grids and for nerfacto's
    // tcnn shapes); otherwise the run-time variant (ND = -1) reads the uploaded table
    const bool use_copies = !alt && f.nd_torch > 0 && (!tcnn || (f.td_main >= 0 && f.td_main <= f.nd_torch));
    const int nd = use_copies && (f.nd_torch == kSnBcMain || f.nd_torch == kSnDenseLevelsDefault) ? f.nd_torch : -1;
    if (r.march_stats) {
        if (half1 || r.dump || alt)
            return refuse("SnRenderOpts.march_stats: no counting instantiation for this variant (single fp16 / instrumented / generic sampler)");
        if (!(split && !tcnn && f.nd_torch == kSnDenseLevelsDefault))
            return refuse("SnRenderOpts.march_stats: the counting instantiation of the main kernel exists for the default variant only (torch grid, 11 de-hashed levels, precision 1)");
    }
    if (mode) {
        const SnPropSelection ps = sn_select_proposal(f, r);
        if (ps.err) return refuse(ps.text);
    }
    auto take = [&](SnMainVariant v, bool hgrid) { return SnMainSelection{SN_OK, "", v, split, half1, use_copies, hgrid}; };
    if (half1) {
        // single fp16: the tiny-cuda-nn grid's kernels (valid_opts).  ND = 11: the grid from its fp16 storage; otherwise the run-time variant
        // on the uploaded fp32 table with every row rounded through fp16 on the fly -- the same values
        if (r.dump || alt) return refuse("precision 2 (single fp16) has no instrumented / generic-sampler instantiation");
        const bool hgrid = nd == kSnDenseLevelsDefault && f.has_half_grid;
        return take({mode, 2, 1, hgrid ? kSnDenseLevelsDefault : -1, false, false, false}, hgrid);
    }
    if (r.dump) {  // instrumented instantiations: the production variant, both samplers, both precisions
        if (tcnn || f.nd_torch != kSnDenseLevelsDefault || alt)
            return refuse("sn_render_rays_debug: the main-kernel dump exists for the default variant only (torch grid, 11 de-hashed levels, default sampler and scene contraction)");
        return take({mode, prec, 0, kSnDenseLevelsDefault, true, false, false}, false);
    }
    if (alt) return take({mode, prec, tcnn, -1, false, true, false}, false);
    if (r.march_stats) return take({mode, 1, 0, kSnDenseLevelsDefault, false, false, true}, false);  // (diagnostics; refused above for every other variant)
    return take({mode, prec, tcnn, nd, false, false, false}, false);
}

// The normals kernel itself refuses nothing; a normals render that samples its own bins takes sn_select_proposal's refusals.  Nerfacto's
// torch grid with its default 11 de-hashed levels reads them (168 gathers per step instead of 256); other shapes and the tiny-cuda-nn grid
// read the uploaded table.
inline SnNormalsSelection sn_select_normals(const SnVariantFacts& f, const SnVariantRequest& r) {
    const bool alt = needs_generic_kernels(f, r), tcnn = f.main_grid_mode == 1;
    const int prec = sn_normals_precision(f, r.precision), mode = r.num_proposal_iterations > 0;
    const bool copies = !alt && !tcnn && f.nd_torch == kSnDenseLevelsDefault && f.has_dense_main;
    return SnNormalsSelection{SN_OK, "", {mode, tcnn, prec, copies ? kSnDenseLevelsDefault : -1, alt}, prec == 1, false, copies, false};
}

// ---- the instantiations that are built: X(template arguments in the kernel's order) -------------------------------------------------
// K1 <MODE, PREC, GRID, ND, DUMP, ALT, STATS>: 42
#define SN_MAIN_VARIANTS_PLAIN(X, MODE, PREC, GRID) \
    X(MODE, PREC, GRID, 9, false, false, false) X(MODE, PREC, GRID, 11, false, false, false) X(MODE, PREC, GRID, -1, false, false, false)
#define SN_MAIN_VARIANTS_MODE(X, MODE)                                                                                \
    SN_MAIN_VARIANTS_PLAIN(X, MODE, 0, 0) SN_MAIN_VARIANTS_PLAIN(X, MODE, 0, 1)                                       \
    SN_MAIN_VARIANTS_PLAIN(X, MODE, 1, 0) SN_MAIN_VARIANTS_PLAIN(X, MODE, 1, 1)                                       \
    X(MODE, 2, 1, 11, false, false, false) X(MODE, 2, 1, -1, false, false, false)           /* single fp16 */         \
    X(MODE, 0, 0, 11, true, false, false) X(MODE, 1, 0, 11, true, false, false)             /* instrumented */        \
    X(MODE, 0, 0, -1, false, true, false) X(MODE, 0, 1, -1, false, true, false)             /* generic */             \
    X(MODE, 1, 0, -1, false, true, false) X(MODE, 1, 1, -1, false, true, false)                                       \
    X(MODE, 1, 0, 11, false, false, true)                                                   /* counting */
#define SN_MAIN_VARIANTS(X) SN_MAIN_VARIANTS_MODE(X, 0) SN_MAIN_VARIANTS_MODE(X, 1)

// K2 <GRID, ND0, ND1, DUMP, ALT, STATS>: 8
#define SN_PROP_VARIANTS(X)                                                     \
    X(0, 5, 4, false, false, false) X(0, -1, -1, false, false, false)           \
    X(1, 5, 4, false, false, false) X(1, -1, -1, false, false, false)           \
    X(0, -1, -1, false, true, false) X(1, -1, -1, false, true, false)           \
    X(0, 5, 4, true, false, false) X(0, 5, 4, false, false, true)

// normals <MODE, GRID, PREC, ND, ALT>: 20
#define SN_NORMALS_VARIANTS_MODE(X, MODE, PREC)                                                              \
    X(MODE, 0, PREC, 11, false) X(MODE, 0, PREC, -1, false) X(MODE, 1, PREC, -1, false)                      \
    X(MODE, 0, PREC, -1, true) X(MODE, 1, PREC, -1, true)
#define SN_NORMALS_VARIANTS(X) \
    SN_NORMALS_VARIANTS_MODE(X, 0, 0) SN_NORMALS_VARIANTS_MODE(X, 0, 1) SN_NORMALS_VARIANTS_MODE(X, 1, 0) SN_NORMALS_VARIANTS_MODE(X, 1, 1)
