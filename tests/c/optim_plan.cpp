// optim_plan.cpp -- the host planner of sn_adam_step (signerf_amd/csrc/sn_optim_plan.h) as a stand-alone program (tests/test_optim_host.py).
//
//     optim_plan check              plans mixed tensor lists (sizes 0, 1, 3, 4, 5, 255, 256, 257, 65539 and a few large ones; fewer and more
//                                   tensors than one launch takes; one to three groups, clipping or not) and holds every plan against its
//                                   invariants; prints the counts
//     optim_plan workspace N TOTAL  prints the workspace layout for N tensors of TOTAL elements: "records partials total"
// Exit status 0 when every check held; failures go to stderr.
#include "../../signerf_amd/csrc/sn_optim_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static int g_failures = 0;
static void failed(const std::string& what) {
    if (++g_failures <= 20) fprintf(stderr, "optim_plan: %s\n", what.c_str());
}
#define HOLD(cond, ...)                                  \
    do {                                                 \
        if (!(cond)) {                                   \
            char text[256];                              \
            snprintf(text, sizeof(text), __VA_ARGS__);   \
            failed(std::string(#cond) + ": " + text);    \
        }                                                \
    } while (0)

struct Counts {
    uint64_t cases = 0, batches = 0, chunks = 0, elements = 0, partials = 0, strided = 0;
};

static void check_case(const std::vector<int64_t>& n, const std::vector<int32_t>& group, const std::vector<uint8_t>& clips, Counts& counts) {
    const int32_t nt = (int32_t)n.size(), ng = (int32_t)clips.size();
    SnAdamPlan plan;
    HOLD(sn_plan_adam(n.data(), group.data(), nt, clips.data(), ng, plan), "%d tensors", nt);
    ++counts.cases;
    int64_t total = 0;
    for (int64_t v : n) total += v;
    // every element exactly once, by the function the kernels call; no chunk crosses its tensor
    std::vector<std::vector<uint8_t>> seen((size_t)nt);
    for (int32_t i = 0; i < nt; ++i) seen[(size_t)i].assign((size_t)n[(size_t)i], 0);
    std::vector<int> batches_of((size_t)nt, 0);
    std::vector<uint8_t> partial_used((size_t)plan.n_partials, 0);
    for (const SnAdamBatch& b : plan.batches) {
        ++counts.batches;
        HOLD(b.n_slots >= 1 && b.n_slots <= kSnAdamMaxTensors, "n_slots %d", b.n_slots);
        HOLD(b.prefix[0] == 0 && b.prefix[b.n_slots] == b.n_chunks, "prefix ends at %u of %u", b.prefix[b.n_slots], b.n_chunks);
        HOLD(b.grid == (b.n_chunks < kSnAdamMaxGrid ? b.n_chunks : kSnAdamMaxGrid) && b.grid >= 1, "grid %u for %u chunks", b.grid, b.n_chunks);
        counts.strided += b.n_chunks > b.grid;
        bool clips_any = false;
        for (int32_t k = 0; k < b.n_slots; ++k) {
            const int32_t i = b.tensor[k];
            HOLD(i >= 0 && i < nt && b.n[k] == n[(size_t)i] && b.n[k] > 0, "slot %d names tensor %d", k, i);
            HOLD(b.prefix[k + 1] - b.prefix[k] == sn_adam_chunks(b.n[k]), "slot %d has %u chunks", k, b.prefix[k + 1] - b.prefix[k]);
            HOLD(k == 0 || b.tensor[k - 1] < i, "slot %d out of the caller's order", k);
            ++batches_of[(size_t)i];
            clips_any = clips_any || clips[(size_t)group[(size_t)i]];
        }
        HOLD(b.clips == clips_any, "batch clips %d", (int)b.clips);
        for (uint32_t c = 0; c < b.n_chunks; ++c) {
            const SnAdamChunkRef r = sn_adam_locate(b.prefix, b.n_slots, b.n, c);
            ++counts.chunks;
            if (!(r.slot >= 0 && r.slot < b.n_slots)) {
                failed("chunk " + std::to_string(c) + " maps to slot " + std::to_string(r.slot));
                continue;
            }
            const int32_t i = b.tensor[r.slot];
            HOLD(r.first >= 0 && r.first % kSnAdamChunk == 0 && r.count >= 1 && r.count <= kSnAdamChunk && r.first + r.count <= n[(size_t)i],
                 "chunk %u = [%lld, +%d) of a tensor of %lld", c, (long long)r.first, r.count, (long long)n[(size_t)i]);
            HOLD(r.count == kSnAdamChunk || r.first + r.count == n[(size_t)i], "a short chunk %u inside tensor %d", c, i);
            if (r.first < 0 || r.first + r.count > n[(size_t)i]) continue;
            for (int32_t e = 0; e < r.count; ++e) ++seen[(size_t)i][(size_t)(r.first + e)];
            if (clips[(size_t)group[(size_t)i]]) {   // where the stats launch writes this chunk's partial sum
                const uint64_t slot = (uint64_t)plan.part_own[(size_t)i] + (c - b.prefix[r.slot]);
                HOLD(slot >= plan.part_lo[(size_t)i] && slot < plan.part_hi[(size_t)i] && slot < plan.n_partials, "partial %llu of tensor %d",
                     (unsigned long long)slot, i);
                if (slot < plan.n_partials) ++partial_used[(size_t)slot];
            }
        }
    }
    for (int32_t i = 0; i < nt; ++i) {
        HOLD(batches_of[(size_t)i] == (n[(size_t)i] > 0 ? 1 : 0), "tensor %d is in %d batches", i, batches_of[(size_t)i]);
        for (uint8_t s : seen[(size_t)i])
            if (s != 1) {
                failed("an element of tensor " + std::to_string(i) + " is covered " + std::to_string((int)s) + " times");
                break;
            }
        counts.elements += (uint64_t)n[(size_t)i];
        if (!clips[(size_t)group[(size_t)i]] || n[(size_t)i] == 0) HOLD(plan.part_lo[(size_t)i] == plan.part_hi[(size_t)i], "tensor %d has partials without clipping", i);
    }
    // the partials: every slot written exactly once, a group's tensors share one range, the ranges of different groups are disjoint
    for (uint8_t u : partial_used)
        if (u != 1) {
            failed("a partial is written " + std::to_string((int)u) + " times");
            break;
        }
    bool any = false;
    for (int32_t i = 0; i < nt; ++i)
        for (int32_t j = 0; j < nt; ++j) {
            const bool ci = clips[(size_t)group[(size_t)i]] && n[(size_t)i] > 0, cj = clips[(size_t)group[(size_t)j]] && n[(size_t)j] > 0;
            any = any || ci;
            if (!ci || !cj) continue;
            if (group[(size_t)i] == group[(size_t)j])
                HOLD(plan.part_lo[(size_t)i] == plan.part_lo[(size_t)j] && plan.part_hi[(size_t)i] == plan.part_hi[(size_t)j], "tensors %d, %d", i, j);
            else
                HOLD(plan.part_hi[(size_t)i] <= plan.part_lo[(size_t)j] || plan.part_hi[(size_t)j] <= plan.part_lo[(size_t)i], "tensors %d, %d", i, j);
        }
    HOLD(plan.any_clip == any, "any_clip %d", (int)plan.any_clip);
    counts.partials += plan.n_partials;
    // the workspace the entry point asks for holds the records and every partial
    const SnAdamWorkspace w = sn_adam_workspace(nt, total);
    HOLD(w.records == 0 && w.partials == (size_t)nt * kSnAdamRecordBytes && w.partials % 8 == 0, "partials at %zu", w.partials);
    HOLD(w.total >= w.partials + (size_t)plan.n_partials * 8, "%zu bytes for %llu partials", w.total, (unsigned long long)plan.n_partials);
    uint64_t all = 0;
    for (int64_t v : n) all += sn_adam_chunks(v);
    HOLD(w.total >= w.partials + all * 8 && w.total == w.partials + ((size_t)total / kSnAdamChunk + (size_t)nt) * 8, "%zu bytes", w.total);
}

static int check() {
    const int64_t sizes[] = {0, 1, 3, 4, 5, 255, 256, 257, 65539};
    const int n_sizes = (int)(sizeof(sizes) / sizeof(sizes[0]));
    Counts counts;
    const uint8_t clip_sets[][3] = {{0, 0, 0}, {1, 1, 1}, {1, 0, 1}, {0, 1, 0}};
    for (int count : {1, 2, 9, kSnAdamMaxTensors - 1, kSnAdamMaxTensors, kSnAdamMaxTensors + 1, 2 * kSnAdamMaxTensors + 7})
        for (int rot = 0; rot < n_sizes; ++rot)
            for (int ng = 1; ng <= 3; ++ng)
                for (const auto& cs : clip_sets) {
                    std::vector<int64_t> n;
                    std::vector<int32_t> group;
                    for (int i = 0; i < count; ++i) {
                        n.push_back(sizes[(i + rot) % n_sizes]);
                        group.push_back((i * 7 + rot) % ng);
                    }
                    check_case(n, group, std::vector<uint8_t>(cs, cs + ng), counts);
                }
    // sizes around a chunk and around a grid's worth of chunks (the grid-stride path), alone and between small tensors
    for (int64_t big : {(int64_t)kSnAdamChunk - 1, (int64_t)kSnAdamChunk, (int64_t)kSnAdamChunk + 1, (int64_t)kSnAdamChunk * kSnAdamMaxGrid - 1,
                        (int64_t)kSnAdamChunk * kSnAdamMaxGrid + 1, (int64_t)1 << 24}) {
        check_case({big}, {0}, {1}, counts);
        check_case({3, big, 0, 257, big, 1}, {0, 1, 1, 0, 0, 1}, {1, 0}, counts);
    }
    check_case({}, {}, {1}, counts);
    check_case({0, 0}, {0, 0}, {1}, counts);
    // the 32-bit chunk numbers: a list that would need more is refused
    {
        SnAdamPlan plan;
        const int64_t n[2] = {(int64_t)kSnAdamChunk << 30, (int64_t)kSnAdamChunk << 30};
        const int32_t g[2] = {0, 0};
        const uint8_t c[1] = {1};
        HOLD(!sn_plan_adam(n, g, 2, c, 1, plan), "2^31 chunks were planned");
        HOLD(sn_plan_adam(n, g, 1, c, 1, plan) && plan.batches.size() == 1 && plan.batches[0].n_chunks == 1u << 30, "2^30 chunks");
    }
    HOLD(sn_adam_workspace(-1, 0).total == 0 && sn_adam_workspace(0, -1).total == 0 && sn_adam_workspace(0, 0).total == 0, "negative arguments");
    printf("cases %llu batches %llu chunks %llu elements %llu partials %llu strided %llu\n", (unsigned long long)counts.cases,
           (unsigned long long)counts.batches, (unsigned long long)counts.chunks, (unsigned long long)counts.elements,
           (unsigned long long)counts.partials, (unsigned long long)counts.strided);
    return g_failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    if (argc == 4 && !strcmp(argv[1], "workspace")) {
        const SnAdamWorkspace w = sn_adam_workspace((int32_t)atoll(argv[2]), (int64_t)atoll(argv[3]));
        printf("%zu %zu %zu\n", w.records, w.partials, w.total);
        return 0;
    }
    fprintf(stderr, "usage: optim_plan check | workspace N TOTAL\n");
    return 2;
}
