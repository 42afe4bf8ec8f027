// sn_api_optim.h (part of sn_api.hip) -- include/signerf_hip_optim.h: the fused Adam step on caller-owned tensors
#pragma once

namespace {

// element i of a caller's array of versioned structs (the stride is the struct_size its elements carry), copied into the library's own
template <typename T>
T adam_element(const T* array, size_t stride, int32_t i) {
    T own;
    memset((void*)&own, 0, sizeof(T));
    memcpy((void*)&own, (const char*)array + stride * (size_t)i, std::min(stride, sizeof(T)));
    return own;
}

// the first element's struct_size, which every element must carry; 0: refused (text set)
template <typename T>
size_t adam_stride(const std::string& who, const T* array, int32_t count, const char* what) {
    uint32_t first = 0;
    memcpy(&first, (const void*)array, sizeof(first));
    if (first != sizeof(T)) {
        fail(nullptr, SN_ERR_INVALID, who + ": " + what + ".struct_size = " + std::to_string(first) + ": this library (SN_OPTIM_ABI_VERSION " +
                                          std::to_string(SN_OPTIM_ABI_VERSION) + ") knows size " + std::to_string(sizeof(T)));
        return 0;
    }
    for (int32_t i = 1; i < count; ++i) {
        uint32_t sz = 0;
        memcpy(&sz, (const char*)array + (size_t)first * (size_t)i, sizeof(sz));
        if (sz != first) {
            fail(nullptr, SN_ERR_INVALID, who + ": " + what + "[" + std::to_string(i) + "].struct_size differs from element 0's");
            return 0;
        }
    }
    return first;
}

}  // namespace

extern "C" {

int sn_optim_abi_version(void) { return SN_OPTIM_ABI_VERSION; }

size_t sn_adam_workspace_bytes(int32_t n_tensors, int64_t total_elements) { return sn_adam_workspace(n_tensors, total_elements).total; }

int sn_adam_step(const SnAdamTensor* tensors, int32_t n_tensors, const SnAdamGroup* groups, int32_t n_groups, const float* grad_scale,
                 const float* found_inf, void* workspace, size_t workspace_bytes, SnStream stream) {
    const std::string who = "sn_adam_step";
    auto refuse = [&](const std::string& text) { return fail(nullptr, SN_ERR_INVALID, who + ": " + text); };
    if (n_tensors < 0 || n_groups < 0) return refuse("n_tensors and n_groups must be >= 0");
    if (n_tensors == 0) return SN_OK;
    if (!tensors || !groups) return refuse("NULL argument (tensors, groups)");
    if (n_groups == 0) return refuse("tensors without a group (n_groups is 0)");
    const size_t t_stride = adam_stride(who, tensors, n_tensors, "SnAdamTensor");
    if (!t_stride) return SN_ERR_INVALID;
    const size_t g_stride = adam_stride(who, groups, n_groups, "SnAdamGroup");
    if (!g_stride) return SN_ERR_INVALID;
    std::vector<SnAdamGroup> G((size_t)n_groups);
    std::vector<uint8_t> clips((size_t)n_groups);
    for (int32_t g = 0; g < n_groups; ++g) {
        const SnAdamGroup& d = G[(size_t)g] = adam_element(groups, g_stride, g);
        const std::string at = "group " + std::to_string(g) + ": ";
        if (!(d.beta1 >= 0.0f && d.beta1 < 1.0f) || !(d.beta2 >= 0.0f && d.beta2 < 1.0f)) return refuse(at + "beta1 and beta2 must lie in [0, 1)");
        if (!(d.eps >= 0.0f)) return refuse(at + "eps must be >= 0");
        if (std::isnan(d.lr) || std::isnan(d.weight_decay) || std::isnan(d.max_norm)) return refuse(at + "lr, weight_decay and max_norm must not be NaN");
        clips[(size_t)g] = d.max_norm > 0.0f;
    }
    std::vector<SnAdamTensor> T((size_t)n_tensors);
    std::vector<int64_t> n((size_t)n_tensors);
    std::vector<int32_t> group((size_t)n_tensors);
    int64_t total = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {
        const SnAdamTensor& d = T[(size_t)i] = adam_element(tensors, t_stride, i);
        const std::string at = "tensor " + std::to_string(i) + ": ";
        if (d.n < 0) return refuse(at + "n must be >= 0");
        if (d.group < 0 || d.group >= n_groups) return refuse(at + "group must lie in [0, n_groups)");
        n[(size_t)i] = d.n;
        group[(size_t)i] = d.group;
        if (d.n == 0) continue;
        if (!d.param || !d.grad || !d.exp_avg || !d.exp_avg_sq || !d.step) return refuse(at + "NULL pointer (param, grad, exp_avg, exp_avg_sq, step)");
        for (const void* q : {(const void*)d.param, (const void*)d.grad, (const void*)d.exp_avg, (const void*)d.exp_avg_sq, (const void*)d.step})
            if ((uintptr_t)q & 3) return refuse(at + "param, grad, exp_avg, exp_avg_sq and step must be aligned to 4 bytes");
        if (d.n > INT64_MAX - total) return refuse("the element total overflows");
        total += d.n;
    }
    if (((uintptr_t)grad_scale | (uintptr_t)found_inf) & 3) return refuse("grad_scale and found_inf must be aligned to 4 bytes");
    if (total == 0) return SN_OK;
    SnAdamPlan plan;
    if (!sn_plan_adam(n.data(), group.data(), n_tensors, clips.data(), n_groups, plan)) return refuse("more than 2^31 chunks of 4096 elements");
    const SnAdamWorkspace ws = sn_adam_workspace(n_tensors, total);
    if (!workspace || workspace_bytes < ws.total)
        return fail(nullptr, SN_ERR_INVALID, who + ": workspace too small, need " + std::to_string(ws.total) + " bytes (sn_adam_workspace_bytes)");
    if ((uintptr_t)workspace & 7) return refuse("the workspace must be aligned to 8 bytes");

    std::vector<SnAdamArgs> args(plan.batches.size());
    for (size_t b = 0; b < plan.batches.size(); ++b) {
        const SnAdamBatch& batch = plan.batches[b];
        SnAdamArgs& a = args[b];
        memset((void*)&a, 0, sizeof(a));
        for (int32_t k = 0; k < batch.n_slots; ++k) {
            const size_t i = (size_t)batch.tensor[k];
            const SnAdamTensor& d = T[i];
            const SnAdamGroup& h = G[(size_t)d.group];
            a.param[k] = d.param;
            a.grad[k] = d.grad;
            a.exp_avg[k] = d.exp_avg;
            a.exp_avg_sq[k] = d.exp_avg_sq;
            a.step[k] = d.step;
            a.n[k] = d.n;
            a.record[k] = (uint32_t)i;
            a.part_own[k] = plan.part_own[i];
            a.part_lo[k] = plan.part_lo[i];
            a.part_hi[k] = plan.part_hi[i];
            a.lr[k] = h.lr;
            a.beta1[k] = h.beta1;
            a.beta2[k] = h.beta2;
            a.eps[k] = h.eps;
            a.weight_decay[k] = h.weight_decay;
            a.max_norm[k] = h.max_norm;
            if ((((uintptr_t)d.param | (uintptr_t)d.grad | (uintptr_t)d.exp_avg | (uintptr_t)d.exp_avg_sq) & 15) == 0) a.vector_mask |= 1u << k;
        }
        memcpy(a.prefix, batch.prefix, sizeof(a.prefix));
        a.n_slots = batch.n_slots;
        a.n_chunks = batch.n_chunks;
        a.grad_scale = grad_scale;
        a.found_inf = found_inf;
        a.records = (SnAdamRecord*)((char*)workspace + ws.records);
        a.partials = (double*)((char*)workspace + ws.partials);
    }
    // all stats launches, then all prologues (a group's partials may come from several launches), then the updates
    const hipStream_t st = (hipStream_t)stream;
    for (size_t b = 0; b < args.size(); ++b)
        if (plan.batches[b].clips) hipLaunchKernelGGL(sn_optim_adam_stats_kernel, dim3(plan.batches[b].grid), dim3(kSnAdamBlock), 0, st, args[b]);
    for (size_t b = 0; b < args.size(); ++b)
        hipLaunchKernelGGL(sn_optim_adam_prologue_kernel, dim3((unsigned)plan.batches[b].n_slots), dim3(kSnAdamBlock), 0, st, args[b]);
    for (size_t b = 0; b < args.size(); ++b)
        hipLaunchKernelGGL(sn_optim_adam_update_kernel, dim3(plan.batches[b].grid), dim3(kSnAdamBlock), 0, st, args[b]);
    return end_launches(who);
}

}  // extern "C"
