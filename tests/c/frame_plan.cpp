// frame_plan.cpp -- the frame plan of signerf_amd/csrc/sn_frame.h as a stand-alone program (tests/test_frame_plan_host.py).
//
//     frame_plan table FILE    one case per line: height width S nprop chunk_rays cus half1 normals_split; prints the case's plan, one line:
//                                  ws=total prop=blocks,threads,ebins,scratch,counter main=grid,lds,ebins,exp_raw,minmax,seg_scratch,n_chunks,
//                                  seg_first_block,n_seg,seg_len combine=n_tail,lds normals=grid,lds tiles=tw_log2,th_log2,tiles_x,tiles_y
//                              with None for what a call does not have (no proposal launch, no tile queue, no bins, no segment jobs)
//     frame_plan enumerate     frames x sample counts x proposal iterations x CU counts: the invariants below on every plan; prints counts,
//                              among them how often plan_tail left a tail whole as "not worth a second kernel"
// Exit status 0 when every check held; failures go to stderr.
#include "../../signerf_amd/csrc/sn_frame.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

static int g_failures = 0;
static void failed(const char* what, int h, int w, int S, int nprop, int cus) {
    if (++g_failures <= 20) fprintf(stderr, "frame_plan: %s at %dx%d S=%d nprop=%d cus=%d\n", what, h, w, S, nprop, cus);
}
#define CHECK(cond) \
    if (!(cond)) failed(#cond, h, w, S, nprop, cus)

static SnRenderOpts opts_of(int S, int nprop, int chunk_rays) {
    SnRenderOpts o;
    memset(&o, 0, sizeof(o));
    o.num_nerf_samples = S;
    o.num_proposal_iterations = nprop;
    o.chunk_rays = chunk_rays;
    return o;
}

static std::string opt(bool have, size_t v) { return have ? std::to_string(v) : "None"; }

static int table(const char* path) {
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        int h, w, S, nprop, chunk, cus, half1, nsplit;
        std::istringstream ss(line);
        if (!(ss >> h >> w >> S >> nprop >> chunk >> cus >> half1 >> nsplit)) return 2;
        const SnFramePlan f = sn_plan_frame(h, w, opts_of(S, nprop, chunk), cus);
        const SnMainLaunch m = sn_main_launch(f, half1 != 0, nprop, false, false);
        const SnNormalsLaunch n = sn_normals_launch(f, nsplit != 0);
        std::string out = "ws=" + std::to_string(f.ws.total) + " prop=";
        if (nprop > 0)
            out += std::to_string(f.prop_blocks) + "," + std::to_string(f.prop_threads) + "," + std::to_string(f.ws.off_ebins) + "," +
                   std::to_string(f.ws.off_prop_scratch) + "," + opt(f.prop_queue, f.ws.off_prop_counter);
        else out += "None";
        out += " main=" + std::to_string(m.grid) + "," + std::to_string(m.lds_bytes) + "," + opt(nprop > 0, f.ws.off_ebins) + "," + std::to_string(f.ws.off_exp_raw) +
               "," + std::to_string(f.ws.off_minmax) + "," + opt(m.n_tail > 0, f.ws.off_seg) + "," + std::to_string(f.ws.n_chunks) + "," +
               std::to_string(m.seg_first_block) + "," + std::to_string(m.n_seg) + "," + std::to_string(m.seg_len);
        out += " combine=" + (m.n_tail > 0 ? std::to_string(m.n_tail) + "," + std::to_string(m.etab_bytes) : std::string("None"));
        out += " normals=" + std::to_string(n.grid) + "," + std::to_string(n.lds_bytes);
        out += " tiles=" + std::to_string(f.g.tw_log2) + "," + std::to_string(f.g.th_log2) + "," + std::to_string(f.g.tiles_x) + "," + std::to_string(f.g.tiles_y);
        puts(out.c_str());
    }
    return 0;
}

static int enumerate() {
    std::set<int> heights, widths;
    for (int h = 1; h <= 40; ++h) heights.insert(h);
    for (int w = 1; w <= 140; ++w) widths.insert(w);
    for (int h : {60, 64, 200, 384, 385, 640, 800}) heights.insert(h);
    for (int w : {200, 512, 640, 800}) widths.insert(w);
    std::vector<int> samples;
    for (int S = 1; S <= 72; ++S) samples.push_back(S);
    for (int S : {96, 128, 255, 256, 257, 512, 1023, 1024}) samples.push_back(S);
    const int chunks[4] = {1, 7, 1000, 1 << 15};
    long plans = 0, split = 0, queued = 0, not_worth = 0, behind_rounds = 0, odd_rows = 0;
    for (int cus : {1, 8, 64, 250, 256, 304})
        for (int h : heights)
            for (int w : widths)
                for (int S : samples)
                    for (int nprop = 0; nprop <= 2; ++nprop) {
                        const SnFramePlan f = sn_plan_frame(h, w, opts_of(S, nprop, chunks[(h + w + S) & 3]), cus);
                        const WorkspacePlan& ws = f.ws;
                        ++plans;
                        // the regions in order, their sizes as the kernels use them: each starts on a multiple of 256 at or behind the end of the one before,
                        // the last one ends at total
                        const size_t n = (size_t)h * w, ntiles = (size_t)f.g.tiles_x * f.g.tiles_y;
                        const size_t tail_wgs = (size_t)(f.total_wgs - f.tail.first_block);
                        const size_t start[6] = {ws.off_exp_raw, ws.off_minmax, ws.off_ebins, ws.off_prop_scratch, ws.off_prop_counter, ws.off_seg};
                        const size_t bytes[6] = {n * 4,
                                                 (size_t)ws.n_chunks * 8,
                                                 nprop ? ntiles * 64 * ((size_t)S + 1) * 4 : 0,
                                                 nprop ? (size_t)f.prop_blocks * SN_PROP_WAVES * SN_PROP_SCRATCH_FLOATS * 4 : 0,
                                                 nprop ? (size_t)4 : 0,
                                                 f.tail.n_seg > 1 ? tail_wgs * 4 * S * 64 * 16 : 0};
                        CHECK(ws.off_exp_raw == 0);
                        for (int r = 0; r < 6; ++r) {
                            CHECK(start[r] % 256 == 0);
                            CHECK(start[r] + bytes[r] <= (r < 5 ? start[r + 1] : ws.total));
                        }
                        CHECK(ws.total % 256 == 0 && ws.total == align256(ws.off_seg + bytes[5]));
                        CHECK((size_t)ws.n_chunks * chunks[(h + w + S) & 3] >= n);
                        CHECK((size_t)f.g.tiles_x << f.g.tw_log2 >= (size_t)w && (size_t)f.g.tiles_y << f.g.th_log2 >= (size_t)h && f.g.tw_log2 + f.g.th_log2 == 6);
                        CHECK(f.total_wgs == f.gbx * f.gby && 2 * f.gbx >= f.g.tiles_x && 2 * f.gby >= f.g.tiles_y);
                        // the tail
                        const int slots = cus * SN_MAIN_WAVES_PER_SIMD;
                        CHECK(f.tail.n_seg >= 1 && (long)f.tail.n_seg * f.tail.seg_len >= S);
                        if (f.tail.n_seg > 1) {
                            ++split;
                            if (f.tail.first_block > 0) ++behind_rounds;
                            CHECK(f.tail.seg_len >= 4 && f.tail.n_seg <= 8);
                            CHECK(f.tail.first_block % 8 == 0 && f.tail.first_block % slots == 0);
                            CHECK(tail_wgs > 0 && tail_wgs <= (size_t)slots / 8);
                        } else {
                            CHECK(f.tail.first_block == f.total_wgs && f.tail.seg_len == S);
                            // which return left it whole: a small tail of S >= 8 samples either is not worth a second kernel, or is and has no whole
                            // rows of 8 in front (the same tail with nothing in front of it is split then)
                            const int tail = f.total_wgs % slots;
                            if (S >= 8 && tail != 0 && tail <= slots / 8) {
                                if (plan_tail(tail, cus, S).n_seg > 1) ++odd_rows;
                                else ++not_worth;
                            }
                        }
                        // the main kernel's launch: whole workgroups plus the tail, padded to rows of 8, times n_seg -- or no segment jobs at all
                        const SnMainLaunch m = sn_main_launch(f, false, nprop, false, false);
                        CHECK(m.grid == (unsigned)(f.tail.first_block + (tail_wgs + 7) / 8 * 8 * (f.tail.n_seg > 1 ? f.tail.n_seg : 0)));
                        CHECK(m.n_seg == f.tail.n_seg && m.seg_len == f.tail.seg_len && m.seg_first_block == f.tail.first_block);
                        CHECK(m.n_tail == (f.tail.n_seg > 1 ? (int)tail_wgs : 0));
                        CHECK(m.etab_bytes == (nprop ? 0 : ((size_t)S + 4) / 4 * 16) && m.etab_bytes % 16 == 0 && (nprop || m.etab_bytes >= ((size_t)S + 1) * 4));
                        CHECK(m.lds_bytes == (size_t)SnMainImg::TOTAL * 4 + m.etab_bytes);
                        for (int off = 0; off < 3; ++off) {   // single fp16, the dump, the switch: whole rays only
                            const SnMainLaunch whole = sn_main_launch(f, off == 0, nprop, off == 1, off == 2);
                            CHECK(whole.grid == (unsigned)f.total_wgs && whole.n_tail == 0 && whole.n_seg == 1 && whole.seg_len == S && whole.seg_first_block == f.total_wgs);
                            CHECK(whole.lds_bytes == (off == 0 ? (size_t)SnMainImgF16::TOTAL_BYTES : (size_t)SnMainImg::TOTAL * 4) + m.etab_bytes);
                        }
                        CHECK(sn_normals_launch(f, false).grid == (unsigned)f.total_wgs && sn_normals_launch(f, true).grid == (unsigned)f.total_wgs);
                        // the proposal launch
                        if (nprop) {
                            CHECK(f.prop_blocks >= 1 && (size_t)f.prop_blocks <= (ntiles + SN_PROP_WAVES - 1) / SN_PROP_WAVES && f.prop_blocks <= 256 * SN_PROP_WG_PER_CU);
                            CHECK(f.prop_threads == 64 * SN_PROP_WAVES && f.prop_queue_start == f.prop_blocks * SN_PROP_WAVES);
                            CHECK(f.prop_queue == (ntiles > (size_t)f.prop_blocks * SN_PROP_WAVES));
                            if (f.prop_queue) ++queued;
                        } else {
                            CHECK(f.prop_blocks == 0 && !f.prop_queue);
                        }
                    }
    printf("plans %ld split %ld behind_full_rounds %ld tile_queue %ld left_whole_no_rows_of_8 %ld left_whole_not_worth %ld\n", plans, split, behind_rounds, queued,
           odd_rows, not_worth);
    return 0;
}

int main(int argc, char** argv) {
    int rc = 2;
    if (argc == 3 && !strcmp(argv[1], "table")) rc = table(argv[2]);
    else if (argc == 2 && !strcmp(argv[1], "enumerate")) rc = enumerate();
    else fprintf(stderr, "usage: frame_plan table FILE | frame_plan enumerate\n");
    return rc ? rc : g_failures ? 1 : 0;
}
