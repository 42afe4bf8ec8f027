// sn_api_hashgrid_tcnn.h (part of sn_api.hip) -- signerf_amd/include/signerf_hip_hashgrid_tcnn.h: the trainable tiny-cuda-nn grid on caller-owned
// tables.  The checks, the parameter block and the launch geometry are sn_api_hashgrid.h's; the kernels are its kernels with the cell
// policy SnHgTcnnGrid (sn_hashgrid_tcnn.h).
#pragma once

static_assert(SN_HASHGRID_TCNN_MAX_LEVELS == SN_HASHGRID_MAX_LEVELS && SN_HASHGRID_TCNN_MAX_LOG2_T == SN_HASHGRID_MAX_LOG2_T,
              "check_hashgrid serves both headers");
static_assert((1u << SN_HASHGRID_TCNN_MAX_LOG2_T) >= SN_TCNN_MAX_RES * SN_TCNN_MAX_RES * SN_TCNN_MAX_RES, "a dense level's r^3 fits its slot");

namespace {

template <int F> struct HgTcnnForward { static constexpr void (*fn)(SnHashgridParams) = sn_hashgrid_forward_kernel<F, SnHgTcnnGrid>; };
template <int F> struct HgTcnnTablePlain { static constexpr void (*fn)(SnHashgridParams) = sn_hashgrid_backward_table_kernel<F, false, SnHgTcnnGrid>; };
template <int F> struct HgTcnnTableMerge { static constexpr void (*fn)(SnHashgridParams) = sn_hashgrid_backward_table_kernel<F, true, SnHgTcnnGrid>; };
template <int F> struct HgTcnnInput { static constexpr void (*fn)(SnHashgridParams) = sn_hashgrid_backward_input_kernel<F, SnHgTcnnGrid>; };

}  // namespace

extern "C" {

int sn_hashgrid_tcnn_abi_version(void) { return SN_HASHGRID_TCNN_ABI_VERSION; }

int sn_hashgrid_tcnn_levels(const float* scalings, int32_t L, int32_t log2_T, int32_t* res, int32_t* rows, int32_t* dense) {
    const std::string who = "sn_hashgrid_tcnn_levels";
    if (L < 1 || L > SN_HASHGRID_TCNN_MAX_LEVELS)
        return fail(nullptr, SN_ERR_INVALID, who + ": L must lie in 1.." + std::to_string(SN_HASHGRID_TCNN_MAX_LEVELS));
    if (log2_T < 1 || log2_T > SN_HASHGRID_TCNN_MAX_LOG2_T)
        return fail(nullptr, SN_ERR_INVALID, who + ": log2_T must lie in 1.." + std::to_string(SN_HASHGRID_TCNN_MAX_LOG2_T));
    if (!scalings) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (scalings)");
    for (int32_t l = 0; l < L; ++l) {
        const SnTcnnLevel lv = sn_tcnn_level(scalings[l], log2_T);
        if (res) res[l] = (int32_t)lv.res;
        if (rows) rows[l] = (int32_t)lv.rows;
        if (dense) dense[l] = lv.dense ? 1 : 0;
    }
    return SN_OK;
}

int sn_hashgrid_tcnn_forward(const float* q, const float* table, const float* scalings, int64_t N, int32_t L, int32_t log2_T, int32_t F,
                             float* enc, int32_t* idx, SnStream stream) {
    const std::string who = "sn_hashgrid_tcnn_forward";
    bool launch;
    if (int rc = check_hashgrid(who, N, L, log2_T, F, q && table && scalings && enc, "q, table, scalings, enc", {table, enc}, idx, &launch)) return rc;
    if (!launch) return SN_OK;
    SnHashgridParams p;
    memset(&p, 0, sizeof(p));
    p.q = q;
    p.table = table;
    p.scal = scalings;
    p.enc = enc;
    p.idx = idx;
    p.N = N;
    p.L = L;
    p.log2_T = log2_T;
    hipLaunchKernelGGL(hashgrid_kernel_for<HgTcnnForward>(F), blocks_for(N * L, SN_HG_BLOCK), dim3(SN_HG_BLOCK), 0, (hipStream_t)stream, p);
    return end_launches(who);
}

int sn_hashgrid_tcnn_backward(const float* q, const float* table, const float* scalings, const float* grad_enc, int64_t N, int32_t L,
                              int32_t log2_T, int32_t F, float* grad_table, float* grad_q, SnStream stream) {
    const std::string who = "sn_hashgrid_tcnn_backward";
    bool launch;
    if (int rc = check_hashgrid(who, N, L, log2_T, F, q && scalings && grad_enc && (grad_table || grad_q) && (table || !grad_q),
                                "q, scalings, grad_enc; grad_table or grad_q; table with grad_q", {table, grad_enc, grad_table}, nullptr, &launch))
        return rc;
    if (!launch) return SN_OK;
    std::call_once(g_hashgrid_env_once, load_hashgrid_env);
    SnHashgridParams p;
    memset(&p, 0, sizeof(p));
    p.q = q;
    p.table = table;
    p.scal = scalings;
    p.grad_enc = grad_enc;
    p.grad_table = grad_table;
    p.grad_q = grad_q;
    p.N = N;
    p.L = L;
    p.log2_T = log2_T;
    p.merge_max_scale = g_hashgrid_tcnn_merge_max_scale.load(std::memory_order_relaxed);
    if (grad_table) {
        const dim3 grid(blocks_for(N, SN_HG_BLOCK).x, (unsigned)L);
        if (p.merge_max_scale >= 0.0f) hipLaunchKernelGGL(hashgrid_kernel_for<HgTcnnTableMerge>(F), grid, dim3(SN_HG_BLOCK), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(hashgrid_kernel_for<HgTcnnTablePlain>(F), grid, dim3(SN_HG_BLOCK), 0, (hipStream_t)stream, p);
    }
    if (grad_q) hipLaunchKernelGGL(hashgrid_kernel_for<HgTcnnInput>(F), blocks_for(N, SN_HG_BLOCK), dim3(SN_HG_BLOCK), 0, (hipStream_t)stream, p);
    return end_launches(who);
}

}  // extern "C"
