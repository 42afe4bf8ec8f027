// sn_optim_plan.h -- the host side of sn_adam_step (include/signerf_hip_optim.h): which (tensor, chunk) every workgroup of the three kinds
// of launch works on, and where they write in the caller's workspace.  Plain C++17, no HIP: tests/c/optim_plan.cpp compiles this header alone.
//   * a CHUNK is kSnAdamChunk consecutive elements of ONE tensor (the last chunk of a tensor may be shorter); it starts a multiple of
//     kSnAdamChunk elements behind the tensor's first, so a chunk of a 16-byte aligned tensor is 16-byte aligned;
//   * a BATCH is what one launch takes: up to kSnAdamMaxTensors tensors with n > 0 in the caller's order, and the prefix table that
//     maps a chunk number of the launch to (tensor, chunk of the tensor) -- sn_adam_locate, the function the kernels call;
//   * the WORKSPACE is one SnAdamRecord-sized slot per element of the caller's array (empty tensors keep theirs, unused), then one fp64
//     partial sum of squares per chunk of every tensor of a clipping group, the chunks of one group side by side in the caller's order:
//     norm_G is the sum of the range [part_lo, part_hi) of the tensor's group, whichever launch holds the tensors.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SN_OPTIM_HD __host__ __device__ inline
#else
#define SN_OPTIM_HD inline
#endif

constexpr int kSnAdamMaxTensors = 32;      // tensors of one launch (SN_ADAM_MAX_TENSORS)
constexpr int kSnAdamBlock = 256;          // lanes of a workgroup
constexpr int kSnAdamChunk = 4096;         // elements of a chunk: four 16-byte accesses per lane
constexpr uint32_t kSnAdamMaxGrid = 2048;  // workgroups of a launch; further chunks are grid-strided
constexpr size_t kSnAdamRecordBytes = 24;  // sizeof(SnAdamRecord)
constexpr uint64_t kSnAdamMaxChunks = 1ull << 31;  // chunk numbers are 32-bit

SN_OPTIM_HD uint64_t sn_adam_chunks(int64_t n) { return n <= 0 ? 0 : ((uint64_t)n + kSnAdamChunk - 1) / kSnAdamChunk; }

struct SnAdamWorkspace {
    size_t records, partials, total;  // byte offsets of the two regions, and the size
};
// an upper bound that needs the tensor count and the element total alone: sum ceil(n_i / C) <= total / C + n_tensors
inline SnAdamWorkspace sn_adam_workspace(int32_t n_tensors, int64_t total_elements) {
    SnAdamWorkspace w{0, 0, 0};
    if (n_tensors < 0 || total_elements < 0) return w;
    w.partials = (size_t)n_tensors * kSnAdamRecordBytes;  // (a multiple of 8)
    w.total = w.partials + ((size_t)total_elements / kSnAdamChunk + (size_t)n_tensors) * sizeof(double);
    return w;
}

// chunk `c` of a launch -> slot k of the launch (the largest k with prefix[k] <= c; prefix[0] = 0, prefix is strictly increasing) and the
// chunk's first element and length in that tensor
struct SnAdamChunkRef {
    int32_t slot;
    int64_t first;
    int32_t count;
};
SN_OPTIM_HD SnAdamChunkRef sn_adam_locate(const uint32_t* prefix, int32_t n_slots, const int64_t* n, uint32_t c) {
    int32_t k = 0;
    for (int32_t j = 1; j < n_slots; ++j) k += prefix[j] <= c ? 1 : 0;
    const int64_t first = (int64_t)(c - prefix[k]) * kSnAdamChunk;
    const int64_t left = n[k] - first;
    return SnAdamChunkRef{k, first, (int32_t)(left < kSnAdamChunk ? left : kSnAdamChunk)};
}

struct SnAdamBatch {
    int32_t n_slots = 0;
    int32_t tensor[kSnAdamMaxTensors] = {};       // slot -> index in the caller's array
    int64_t n[kSnAdamMaxTensors] = {};
    uint32_t prefix[kSnAdamMaxTensors + 1] = {};  // chunks of the launch before slot k; prefix[n_slots] = all of them
    uint32_t n_chunks = 0, grid = 0;
    bool clips = false;                           // some tensor of it belongs to a clipping group: the batch has a stats launch
};

struct SnAdamPlan {
    std::vector<SnAdamBatch> batches;
    std::vector<uint32_t> part_own, part_lo, part_hi;  // per element of the caller's array: its first partial, its group's range (lo == hi: no clipping)
    uint64_t n_partials = 0;
    bool any_clip = false;
};

// n[i], group[i] (already checked: n >= 0, 0 <= group < n_groups), group_clips[g] != 0: max_norm > 0.  false: too many chunks for 32-bit numbers.
inline bool sn_plan_adam(const int64_t* n, const int32_t* group, int32_t n_tensors, const uint8_t* group_clips, int32_t n_groups, SnAdamPlan& plan) {
    plan = SnAdamPlan();
    plan.part_own.assign((size_t)n_tensors, 0u);
    plan.part_lo.assign((size_t)n_tensors, 0u);
    plan.part_hi.assign((size_t)n_tensors, 0u);
    // the partials, group-major: count per group, prefix, then hand out in the caller's order
    std::vector<uint64_t> per_group((size_t)n_groups + 1, 0);
    uint64_t all_chunks = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {
        all_chunks += sn_adam_chunks(n[i]);
        if (group_clips[group[i]]) per_group[(size_t)group[i] + 1] += sn_adam_chunks(n[i]);
    }
    if (all_chunks >= kSnAdamMaxChunks) return false;
    for (int32_t g = 0; g < n_groups; ++g) per_group[(size_t)g + 1] += per_group[(size_t)g];
    plan.n_partials = per_group[(size_t)n_groups];
    std::vector<uint64_t> next(per_group.begin(), per_group.end() - 1);
    for (int32_t i = 0; i < n_tensors; ++i) {
        const int32_t g = group[i];
        if (!group_clips[g] || n[i] == 0) continue;
        plan.any_clip = true;
        plan.part_own[(size_t)i] = (uint32_t)next[(size_t)g];
        next[(size_t)g] += sn_adam_chunks(n[i]);
        plan.part_lo[(size_t)i] = (uint32_t)per_group[(size_t)g];
        plan.part_hi[(size_t)i] = (uint32_t)per_group[(size_t)g + 1];
    }
    // the batches
    for (int32_t i = 0; i < n_tensors; ++i) {
        if (n[i] == 0) continue;
        if (plan.batches.empty() || plan.batches.back().n_slots == kSnAdamMaxTensors) plan.batches.emplace_back();
        SnAdamBatch& b = plan.batches.back();
        const int32_t k = b.n_slots++;
        b.tensor[k] = i;
        b.n[k] = n[i];
        b.prefix[k + 1] = b.prefix[k] + (uint32_t)sn_adam_chunks(n[i]);
        b.n_chunks = b.prefix[k + 1];
        b.grid = b.n_chunks < kSnAdamMaxGrid ? b.n_chunks : kSnAdamMaxGrid;
        b.clips = b.clips || group_clips[group[i]] != 0;
    }
    return true;
}
