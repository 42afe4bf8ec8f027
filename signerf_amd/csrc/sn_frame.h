// sn_frame.h -- the geometry one render call's launches rest on: tiles, the workgroup grid, every offset the three fused kernels write
// to in the caller's workspace (and so the size sn_workspace_bytes promises), the proposal launch, the split-depth tail of the main
// kernel, and the launch arithmetic of the main and the normals kernel.  Plain C++17, no HIP: tests/c/frame_plan.cpp compiles this
// header alone, prints it against the plans recorded from the commit that still computed them inside sn_api.hip
// (tests/golden/frame_plans.json) and enumerates it; tests/test_frame_plan_host.py holds what sn_api.hip launches against the same file.
#pragma once
#include "../../include/signerf_hip.h"
#include "sn_layout.h"

#include <algorithm>
#include <cstddef>

struct TileGeom {
    int tw_log2, th_log2, tiles_x, tiles_y;
};

inline TileGeom tile_geometry(int height, int width) {
    TileGeom g;
    if (height >= 8) {
        g.tw_log2 = 3;
        g.th_log2 = 3;
    } else {
        g.tw_log2 = 6;
        g.th_log2 = 0;
    }
    g.tiles_x = (width + (1 << g.tw_log2) - 1) >> g.tw_log2;
    g.tiles_y = (height + (1 << g.th_log2) - 1) >> g.th_log2;
    return g;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Split-depth tail of the main kernel (sn_main.h SnMainParams).  A launch is whole workgroups (2x2 tiles, 4 waves) on a fixed number of
// slots (CUs x SN_MAIN_WAVES_PER_SIMD workgroups = 768): its last round may hold a handful of workgroups -- a 64x64 viewer frame is 16 of
// them, the tail of a 640x640 frame 64 -- each still marching all S samples with the chip nearly empty.  Such a tail's workgroups are cut
// into n segment jobs of ceil(S / n) samples, so that the round fills more of the chip and is ~1/n as long; a small kernel composites
// the stored samples in order (bit-identical).
// WHEN (measured r03, frames back to back on one stream, profiles/r03_tail_split.txt): it pays when the tail is SMALL -- at most 1/8 of
// the slots: 64x64 0.79 -> 0.25 ms, 128x128 0.69 -> 0.41, 640x640 2.06 -> 1.88 (-9 %).  A tail that already fills a quarter of the chip
// gains nothing or loses: its lone waves step ~2x faster than waves that share a SIMD AND run at the boost clock (the chip is power-
// limited when full), segment jobs pay the prologue n times -- 800x800 (196 of 768) -1 % per launch but +1 % with two frames in flight,
// 200x200 (169) +11 %, 512x512 (256) +8 %.  So: tails above slots / 8 stay whole.
// n minimises a cost model in units of sample steps: rounds of jobs x (samples per job + ~1.5 steps of prologue), a partly filled round
// priced at 0.25 + 0.75 x fill.
struct TailPlan {
    int first_block, n_seg, seg_len;  // (n_seg <= 1: none, first_block = all workgroups)
};
inline TailPlan plan_tail(int total_wgs, int n_cus, int S) {
    TailPlan t{total_wgs, 1, S};
    const int slots = n_cus * SN_MAIN_WAVES_PER_SIMD;
    if (slots <= 0 || S < 8) return t;
    const int tail = total_wgs % slots;
    if (tail == 0 || tail > slots / 8) return t;
    auto cost = [&](int n) {
        const long jobs = (long)tail * n;
        const double len = (double)((S + n - 1) / n) + 1.5;
        const long full = jobs / slots, rest = jobs % slots;
        return (double)full * len + (rest ? len * (0.25 + 0.75 * (double)rest / slots) : 0.0) + 0.5 * (n - 1);  // (+ a little per extra segment: scratch, launch)
    };
    int best = 1;
    double best_cost = cost(1);
    for (int n = 2; n <= 8 && (S + n - 1) / n >= 4; ++n)
        if (cost(n) < best_cost - 1e-9) {
            best = n;
            best_cost = cost(n);
        }
    if (best == 1 || best_cost > 0.9 * cost(1)) return t;  // not worth a second kernel
    t.first_block = total_wgs - tail;
    if (t.first_block % 8 != 0) return TailPlan{total_wgs, 1, S};  // (the XCD-affine job order needs whole rows of 8 in front; true for 256 CUs)
    t.n_seg = best;
    t.seg_len = (S + best - 1) / best;
    return t;
}

// The persistent proposal waves are sized for a chip of this many CUs whatever the device reports: the literal the launch has always
// used.  The workspace a caller sized on one device therefore holds the same proposal scratch on every other.
constexpr int kSnPropGridCus = 256;

// byte offsets into the caller's workspace, each a multiple of 256, in this order; a region a call does not use is empty
struct WorkspacePlan {
    size_t off_exp_raw, off_minmax, off_ebins, off_prop_scratch, off_prop_counter, off_seg, total;
    int n_chunks;
};

struct SnFramePlan {
    int height, width, n_samples;
    TileGeom g;
    int gbx, gby, total_wgs;  // workgroups of 2x2 tiles: the grid of the main kernel's whole-ray jobs and of the normals kernel
    WorkspacePlan ws;
    int prop_blocks, prop_threads;  // the proposal launch (no proposal iterations: 0 blocks)
    bool prop_queue;                // its tile queue (sn_proposal.h): only when some wave gets more than one tile ...
    int prop_queue_start;           // ... and the value the queue's counter starts from: the number of waves
    TailPlan tail;                  // as planned; sn_main_launch decides whether a call uses it
};

// (the size with the tail split planned covers both settings of SN_TAIL_SPLIT)
inline SnFramePlan sn_plan_frame(int height, int width, const SnRenderOpts& o, int n_cus) {
    SnFramePlan f{};
    f.height = height;
    f.width = width;
    f.n_samples = o.num_nerf_samples;
    const size_t n = (size_t)height * width;
    const TileGeom g = f.g = tile_geometry(height, width);
    WorkspacePlan& w = f.ws;
    size_t off = 0;
    w.off_exp_raw = off;
    off += align256(n * 4);
    w.n_chunks = (int)((n + (size_t)o.chunk_rays - 1) / (size_t)o.chunk_rays);
    w.off_minmax = off;
    off += align256((size_t)w.n_chunks * 8);
    w.off_ebins = off;
    w.off_prop_scratch = off;
    w.off_prop_counter = off;
    f.prop_threads = 64 * SN_PROP_WAVES;
    if (o.num_proposal_iterations > 0) {
        off += align256((size_t)g.tiles_x * g.tiles_y * 64 * (o.num_nerf_samples + 1) * 4);
        // persistent proposal waves: what the chip holds (kSnPropGridCus x SN_PROP_WG_PER_CU workgroups of SN_PROP_WAVES waves), at most one per tile
        const int ntiles = g.tiles_x * g.tiles_y;
        f.prop_blocks = std::min((ntiles + SN_PROP_WAVES - 1) / SN_PROP_WAVES, kSnPropGridCus * SN_PROP_WG_PER_CU);
        f.prop_queue_start = f.prop_blocks * SN_PROP_WAVES;
        f.prop_queue = ntiles > f.prop_queue_start;
        w.off_prop_scratch = off;
        off += align256((size_t)f.prop_blocks * SN_PROP_WAVES * SN_PROP_SCRATCH_FLOATS * 4);
        w.off_prop_counter = off;   // the proposal kernel's tile queue (one uint32, set per launch)
        off += 256;
    }
    f.gbx = (g.tiles_x + 1) / 2;
    f.gby = (g.tiles_y + 1) / 2;
    f.total_wgs = f.gbx * f.gby;
    f.tail = plan_tail(f.total_wgs, n_cus, o.num_nerf_samples);
    w.off_seg = off;
    if (f.tail.n_seg > 1) off += align256((size_t)(f.total_wgs - f.tail.first_block) * 4 * (size_t)o.num_nerf_samples * 64 * 16);  // (density, r, g, b) per sample
    w.total = off;
    return f;
}

// The main kernel's launch.  The planned tail is used unless the call dumps, runs the single-fp16 form or has the split switched off;
// then workgroups [0, seg_first_block) march whole rays and the n_tail workgroups behind them become n_seg segment jobs each, the tail
// padded to whole XCD rows of 8 (sn_main.h decodes a segment job from exactly this grid).  n_tail > 0 says that the split is on.
struct SnMainLaunch {
    unsigned grid;
    size_t lds_bytes, etab_bytes;  // weight image + (uniform sampler) the frame's S + 1 euclidean bins
    int n_tail;
    int seg_first_block, n_seg, seg_len;  // SnMainParams
};
inline SnMainLaunch sn_main_launch(const SnFramePlan& f, bool half1, int nprop, bool dump, bool tail_split_off) {
    SnMainLaunch m{};
    m.etab_bytes = nprop == 0 ? ((size_t)f.n_samples + 1 + 3) / 4 * 16 : 0;
    m.lds_bytes = (half1 ? (size_t)SnMainImgF16::TOTAL_BYTES : (size_t)SnMainImg::TOTAL * 4) + m.etab_bytes;
    const bool tail_split = !dump && !half1 && !tail_split_off && f.tail.n_seg > 1;
    m.seg_first_block = f.total_wgs;
    m.n_seg = 1;
    m.seg_len = f.n_samples;
    if (tail_split) {
        m.n_tail = f.total_wgs - f.tail.first_block;
        m.seg_first_block = f.tail.first_block;
        m.n_seg = f.tail.n_seg;
        m.seg_len = f.tail.seg_len;
    }
    m.grid = (unsigned)(f.total_wgs - m.n_tail + ((m.n_tail + 7) / 8 * 8) * m.n_seg);
    return m;
}

struct SnNormalsLaunch {
    unsigned grid;
    size_t lds_bytes;
};
inline SnNormalsLaunch sn_normals_launch(const SnFramePlan& f, bool split) {
    return SnNormalsLaunch{(unsigned)f.total_wgs, split ? (size_t)SnNormImgH::TOTAL_BYTES : (size_t)SnNormImg::TOTAL * 4};
}
