// sn_wide.h -- the host side of a WIDE main field (hidden_dim = hidden_dim_color = 128; kernels: sn_wide_kernels.h): which of the four
// instantiations of sn_wide_field_main_kernel a render call launches or why it is refused, and the launch arithmetic.  Plain C++17, no HIP, like
// sn_variant.h and sn_frame.h: tests/c/wide_pack.cpp compiles this header alone and prints the selector's whole table.
//
// A wide handle renders in exact fp32 whatever precision is asked for (sn_effective_precision says so; precision 2 is refused: its
// arithmetic is not built), reads the uploaded hash table only (no de-hashed copies, no x-paired tables, no fp16 grid) and has no
// instrumented, counting or normals kernels.  The proposal nets are nerfacto's own: sn_select_proposal applies unchanged.
#pragma once
#include "sn_frame.h"
#include "sn_variant.h"

// the (hidden_dim, hidden_dim_color) pairs sn_create accepts
constexpr int kSnFieldWidths[2] = {64, 128};
inline bool sn_width_pair_supported(int hidden_dim, int hidden_dim_color) {
    return hidden_dim == hidden_dim_color && (hidden_dim == kSnFieldWidths[0] || hidden_dim == kSnFieldWidths[1]);
}
constexpr const char* kSnWidthPairsText =
    "supported (hidden_dim, hidden_dim_color) pairs of the main field: (64, 64) and (128, 128)";

// template arguments of sn_wide_field_main_kernel<MODE, GRID>
struct SnWideMainVariant { int mode, grid; };
using SnWideMainSelection = SnSelection<SnWideMainVariant>;

constexpr const char* kSnWideNoHalf = "wide field (hidden_dim 128): precision 2 (single fp16) is not built; wide fields render in exact fp32";
constexpr const char* kSnWideNoDump = "wide field (hidden_dim 128): sn_render_rays_debug is not built (no instrumented instantiation of the wide kernel)";
constexpr const char* kSnWideNoStats = "wide field (hidden_dim 128): SnRenderOpts.march_stats is not built (no counting instantiation of the wide kernel)";
constexpr const char* kSnWideNoNormals = "wide field (hidden_dim 128): sn_render_normals is not built (no normals kernel for wide fields)";

// Every refusal of a colour render on a wide handle, then the instantiation.  The one kernel per (MODE, GRID) serves both samplers, both
// position maps and every far plane (strict position arithmetic); a render with proposal iterations takes the proposal kernel's refusals.
inline SnWideMainSelection sn_select_main_wide(const SnVariantFacts& f, const SnVariantRequest& r) {
    auto refuse = sn_refuse<SnWideMainVariant>;
    if (r.precision == 2) return refuse(kSnWideNoHalf);
    if (r.dump) return refuse(kSnWideNoDump);
    if (r.march_stats) return refuse(kSnWideNoStats);
    const int mode = r.num_proposal_iterations > 0;
    if (mode) {
        const SnPropSelection ps = sn_select_proposal(f, r);
        if (ps.err) return refuse(ps.text);
    }
    return SnWideMainSelection{SN_OK, "", {mode, f.main_grid_mode == 1}, false, false, false, false};
}

// what a wide handle answers sn_effective_precision: exact fp32 for every supported request
inline int sn_effective_precision_wide(const SnVariantFacts& f, int requested, int kernel) {
    if ((kernel != 0 && kernel != 1) || !sn_precision_supported(f.main_grid_mode, requested)) return -1;
    return 0;
}

// sn_wide_field_main_kernel <MODE, GRID>: 4
#define SN_WIDE_MAIN_VARIANTS(X) X(0, 0) X(0, 1) X(1, 0) X(1, 1)

// The wide kernel's launch: whole-ray workgroups only (no split-depth tail); LDS = the image + (uniform sampler) the S + 1 bins.
// More than 64 KiB of dynamic LDS: the launcher raises the kernel's limit first (hipFuncSetAttribute), on a wide handle's path only.
struct SnWideLaunch {
    unsigned grid;
    size_t lds_bytes, etab_bytes;
};
inline SnWideLaunch sn_wide_main_launch(const SnFramePlan& f, int nprop) {
    SnWideLaunch m{};
    m.etab_bytes = nprop == 0 ? ((size_t)f.n_samples + 1 + 3) / 4 * 16 : 0;
    m.lds_bytes = (size_t)SnWideImg::TOTAL * 4 + m.etab_bytes;
    m.grid = (unsigned)f.total_wgs;
    return m;
}
constexpr size_t kSnWideMaxLdsBytes = (size_t)(SnWideImg::TOTAL + SnWideImg::MAX_BINS) * 4;
