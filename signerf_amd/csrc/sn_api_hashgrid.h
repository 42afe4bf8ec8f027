// sn_api_hashgrid.h (part of sn_api.hip) -- include/signerf_hip_hashgrid.h: the trainable hash grid on caller-owned tables
#pragma once

static_assert(SN_HASHGRID_MAX_LEVELS <= 65535, "the level is the grid's y index");

namespace {

// backward_table's merged form (sn_hashgrid.h, variant B) serves the levels with scale <= this; negative: none.  The default is what
// the same-box A/B of tools/hashgrid_bench.py showed (DESIGN.md §4 "Trainable hash grid", "A/B"): on ray-ordered samples every level up to
// scale 128..212 gains (a proposal level at 256 samples per ray 1.4x..1.7x each), the levels above 256 neither gain nor lose.
constexpr float kSnHashgridMergeMaxScale = 256.0f;
std::atomic<float> g_hashgrid_merge_max_scale{kSnHashgridMergeMaxScale};
// the same threshold for the tiny-cuda-nn grid (sn_api_hashgrid_tcnn.h), whose scales are res - 1 and whose coarse levels are dense: the
// sweep of tools/hashgrid_bench.py --grid tcnn (DESIGN.md §4 "Trainable tcnn grid", "A/B").  The variable overrides both.
constexpr float kSnHashgridTcnnMergeMaxScale = 256.0f;
std::atomic<float> g_hashgrid_tcnn_merge_max_scale{kSnHashgridTcnnMergeMaxScale};
std::once_flag g_hashgrid_env_once;

void load_hashgrid_env() {
    const char* e = getenv("SN_HASHGRID_MERGE_MAX_SCALE");
    g_hashgrid_merge_max_scale = e ? (float)atof(e) : kSnHashgridMergeMaxScale;
    g_hashgrid_tcnn_merge_max_scale = e ? (float)atof(e) : kSnHashgridTcnnMergeMaxScale;
}

// the checks both entry points share, in this order; *launch says whether anything is left to do
int check_hashgrid(const std::string& who, int64_t N, int32_t L, int32_t log2_T, int32_t F, bool pointers_ok, const char* pointers,
                   std::initializer_list<const void*> rows, const void* idx, bool* launch) {
    *launch = false;
    if (N < 0) return fail(nullptr, SN_ERR_INVALID, who + ": N must be >= 0");
    if (L < 1 || L > SN_HASHGRID_MAX_LEVELS) return fail(nullptr, SN_ERR_INVALID, who + ": L must lie in 1.." + std::to_string(SN_HASHGRID_MAX_LEVELS));
    if (log2_T < 1 || log2_T > SN_HASHGRID_MAX_LOG2_T)
        return fail(nullptr, SN_ERR_INVALID, who + ": log2_T must lie in 1.." + std::to_string(SN_HASHGRID_MAX_LOG2_T));
    if (F != 1 && F != 2 && F != 4 && F != 8) return fail(nullptr, SN_ERR_INVALID, who + ": F must be 1, 2, 4 or 8");
    if (((uint64_t)L << log2_T) * (uint64_t)F >= (1ull << 31))
        return fail(nullptr, SN_ERR_INVALID, who + ": L * 2^log2_T * F must stay below 2^31 table elements (32-bit element offsets)");
    if (N == 0) return SN_OK;
    if (!pointers_ok) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (" + pointers + ")");
    if (N > 0x7fffffffll) return fail(nullptr, SN_ERR_INVALID, who + ": N exceeds the grid (2^31 - 1 points)");
    const uintptr_t row_mask = (uintptr_t)std::min(4 * F, 16) - 1;
    for (const void* r : rows)
        if ((uintptr_t)r & row_mask) return fail(nullptr, SN_ERR_INVALID, who + ": table, enc, grad_enc and grad_table must be aligned to min(4 F, 16) bytes");
    if ((uintptr_t)idx & 15) return fail(nullptr, SN_ERR_INVALID, who + ": idx must be aligned to 16 bytes");
    *launch = true;
    return SN_OK;
}

template <template <int> class K>
auto hashgrid_kernel_for(int32_t F) {
    return F == 1 ? K<1>::fn : F == 2 ? K<2>::fn : F == 4 ? K<4>::fn : K<8>::fn;
}
template <int F> struct HgForward { static constexpr void (*fn)(SnHashgridParams) = sn_hashgrid_forward_kernel<F>; };
template <int F> struct HgTablePlain { static constexpr void (*fn)(SnHashgridParams) = sn_hashgrid_backward_table_kernel<F, false>; };
template <int F> struct HgTableMerge { static constexpr void (*fn)(SnHashgridParams) = sn_hashgrid_backward_table_kernel<F, true>; };
template <int F> struct HgInput { static constexpr void (*fn)(SnHashgridParams) = sn_hashgrid_backward_input_kernel<F>; };

}  // namespace

extern "C" {

int sn_hashgrid_abi_version(void) { return SN_HASHGRID_ABI_VERSION; }

int sn_hashgrid_debug_reload_env(void) {
    std::call_once(g_hashgrid_env_once, [] {});
    load_hashgrid_env();
    return SN_OK;
}

int sn_hashgrid_forward(const float* q, const float* table, const float* scalings, int64_t N, int32_t L, int32_t log2_T, int32_t F,
                        float* enc, int32_t* idx, SnStream stream) {
    const std::string who = "sn_hashgrid_forward";
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
    hipLaunchKernelGGL(hashgrid_kernel_for<HgForward>(F), blocks_for(N * L, SN_HG_BLOCK), dim3(SN_HG_BLOCK), 0, (hipStream_t)stream, p);
    return end_launches(who);
}

int sn_hashgrid_backward(const float* q, const float* table, const float* scalings, const float* grad_enc, int64_t N, int32_t L,
                         int32_t log2_T, int32_t F, float* grad_table, float* grad_q, SnStream stream) {
    const std::string who = "sn_hashgrid_backward";
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
    p.merge_max_scale = g_hashgrid_merge_max_scale.load(std::memory_order_relaxed);
    if (grad_table) {
        const dim3 grid(blocks_for(N, SN_HG_BLOCK).x, (unsigned)L);
        if (p.merge_max_scale >= 0.0f) hipLaunchKernelGGL(hashgrid_kernel_for<HgTableMerge>(F), grid, dim3(SN_HG_BLOCK), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(hashgrid_kernel_for<HgTablePlain>(F), grid, dim3(SN_HG_BLOCK), 0, (hipStream_t)stream, p);
    }
    if (grad_q) hipLaunchKernelGGL(hashgrid_kernel_for<HgInput>(F), blocks_for(N, SN_HG_BLOCK), dim3(SN_HG_BLOCK), 0, (hipStream_t)stream, p);
    return end_launches(who);
}

}  // extern "C"
