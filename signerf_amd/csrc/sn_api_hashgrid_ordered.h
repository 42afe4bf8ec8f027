// sn_api_hashgrid_ordered.h (part of sn_api.hip) -- signerf_amd/include/signerf_hip_hashgrid_ordered.h: the ordered (store, sort, sum) form
// of the table gradient of both trainable grids.  The checks and the parameter block are sn_api_hashgrid.h's; the kernels are
// sn_hashgrid_ordered.h's, and grad_q comes from sn_hashgrid_backward_input_kernel as in the atomic entry points.
#pragma once

static_assert(SN_HASHGRID_ORDERED_MAX_POINTS == (1ll << 28) - 1, "8 N contribution ids fit 31 bits");

namespace {

// the workspace of ONE level, reused by every level: a function of (N, F) alone
struct HgOrderedLayout {
    size_t vals, keys[2], ids[2], hist, totals, bytes;
    uint32_t M, tiles;
};

HgOrderedLayout hashgrid_ordered_layout(int64_t N, int32_t F) {
    HgOrderedLayout w;
    const size_t M = (size_t)N * 8;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    w.M = (uint32_t)M;
    w.tiles = (uint32_t)((M + SN_HGO_TILE - 1) / SN_HGO_TILE);
    size_t at = 0;
    w.vals = at, at += up(M * (size_t)F * sizeof(float));
    for (int i = 0; i < 2; ++i) w.keys[i] = at, at += up(M * sizeof(uint32_t));
    for (int i = 0; i < 2; ++i) w.ids[i] = at, at += up(M * sizeof(uint32_t));
    w.hist = at, at += up((size_t)SN_HGO_BINS * w.tiles * sizeof(uint32_t));
    w.totals = at, at += up(SN_HGO_BINS * sizeof(uint32_t));
    w.bytes = at;
    return w;
}

bool hashgrid_ordered_shape_ok(int64_t N, int32_t L, int32_t log2_T, int32_t F) {
    return N > 0 && N <= SN_HASHGRID_ORDERED_MAX_POINTS && L >= 1 && L <= SN_HASHGRID_MAX_LEVELS && log2_T >= 1 && log2_T <= SN_HASHGRID_MAX_LOG2_T &&
           (F == 1 || F == 2 || F == 4 || F == 8) && ((uint64_t)L << log2_T) * (uint64_t)F < (1ull << 31);
}

template <int F> struct HgOrderedEmit { static constexpr void (*fn)(SnHgOrderedParams) = sn_hashgrid_ordered_emit_kernel<F, SnHgTorchGrid>; };
template <int F> struct HgOrderedEmitTcnn { static constexpr void (*fn)(SnHgOrderedParams) = sn_hashgrid_ordered_emit_kernel<F, SnHgTcnnGrid>; };
template <int F> struct HgOrderedSum { static constexpr void (*fn)(SnHgOrderedParams) = sn_hashgrid_ordered_segment_sum_kernel<F>; };

template <template <int> class K>
auto hashgrid_ordered_kernel_for(int32_t F) {
    return F == 1 ? K<1>::fn : F == 2 ? K<2>::fn : F == 4 ? K<4>::fn : K<8>::fn;
}

template <template <int> class Emit, template <int> class Input>
int hashgrid_ordered_backward(const std::string& who, const float* q, const float* table, const float* scalings, const float* grad_enc, int64_t N,
                              int32_t L, int32_t log2_T, int32_t F, float* grad_table, float* grad_q, void* workspace, size_t workspace_bytes,
                              SnStream stream) {
    bool launch;
    if (int rc = check_hashgrid(who, N, L, log2_T, F, q && scalings && grad_enc && (grad_table || grad_q) && (table || !grad_q),
                                "q, scalings, grad_enc; grad_table or grad_q; table with grad_q", {table, grad_enc, grad_table}, nullptr, &launch))
        return rc;
    if (!launch) return SN_OK;
    HgOrderedLayout w{};
    if (grad_table) {   // (a grad_q-only call forms no contribution ids: it takes what the atomic entry point takes)
        if (N > SN_HASHGRID_ORDERED_MAX_POINTS)
            return fail(nullptr, SN_ERR_INVALID, who + ": with grad_table N must stay below 2^28 points (the 8 N contribution ids of a level are 32-bit)");
        w = hashgrid_ordered_layout(N, F);
        if (!workspace) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (workspace, required with grad_table)");
        if ((uintptr_t)workspace & 15) return fail(nullptr, SN_ERR_INVALID, who + ": workspace must be aligned to 16 bytes");
        if (workspace_bytes < w.bytes)
            return fail(nullptr, SN_ERR_INVALID, who + ": workspace of " + std::to_string(workspace_bytes) + " bytes, sn_hashgrid_ordered_workspace_bytes asks for " +
                                                     std::to_string(w.bytes));
    }
    const hipStream_t s = (hipStream_t)stream;
    SnHgOrderedParams p;
    memset(&p, 0, sizeof(p));
    p.g.q = q;
    p.g.table = table;
    p.g.scal = scalings;
    p.g.grad_enc = grad_enc;
    p.g.grad_table = grad_table;
    p.g.grad_q = grad_q;
    p.g.N = N;
    p.g.L = L;
    p.g.log2_T = log2_T;
    if (grad_table) {
        char* base = (char*)workspace;
        uint32_t* keys[2] = {(uint32_t*)(base + w.keys[0]), (uint32_t*)(base + w.keys[1])};
        uint32_t* ids[2] = {(uint32_t*)(base + w.ids[0]), (uint32_t*)(base + w.ids[1])};
        p.vals = (float*)(base + w.vals);
        p.hist = (uint32_t*)(base + w.hist);
        p.totals = (uint32_t*)(base + w.totals);
        p.M = w.M;
        p.tiles = w.tiles;
        const int passes = (log2_T + 7) / 8;
        const dim3 block(SN_HGO_BLOCK);
        for (int32_t l = 0; l < L; ++l) {   // one level at a time: the stream orders the reuse of the workspace
            p.level = l;
            p.keys_out = keys[0];
            hipLaunchKernelGGL(hashgrid_ordered_kernel_for<Emit>(F), blocks_for(N, SN_HGO_BLOCK), block, 0, s, p);
            for (int pass = 0; pass < passes; ++pass) {
                p.shift = 8 * pass;
                p.keys_in = keys[pass & 1];
                p.ids_in = ids[pass & 1];
                p.keys_out = keys[(pass + 1) & 1];
                p.ids_out = ids[(pass + 1) & 1];
                hipLaunchKernelGGL(sn_hashgrid_ordered_histogram_kernel, dim3(w.tiles), block, 0, s, p);
                hipLaunchKernelGGL(sn_hashgrid_ordered_scan_digit_kernel, dim3(SN_HGO_BINS), block, 0, s, p);
                if (pass == 0) hipLaunchKernelGGL(sn_hashgrid_ordered_scatter_kernel<true>, dim3(w.tiles), block, 0, s, p);
                else hipLaunchKernelGGL(sn_hashgrid_ordered_scatter_kernel<false>, dim3(w.tiles), block, 0, s, p);
            }
            p.keys_in = keys[passes & 1];
            p.ids_in = ids[passes & 1];
            hipLaunchKernelGGL(hashgrid_ordered_kernel_for<HgOrderedSum>(F), blocks_for((int64_t)w.M, SN_HGO_BLOCK), block, 0, s, p);
        }
    }
    if (grad_q) hipLaunchKernelGGL(hashgrid_kernel_for<Input>(F), blocks_for(N, SN_HG_BLOCK), dim3(SN_HG_BLOCK), 0, s, p.g);
    return end_launches(who);
}

}  // namespace

extern "C" {

int sn_hashgrid_ordered_abi_version(void) { return SN_HASHGRID_ORDERED_ABI_VERSION; }

size_t sn_hashgrid_ordered_workspace_bytes(int64_t N, int32_t L, int32_t log2_T, int32_t F) {
    return hashgrid_ordered_shape_ok(N, L, log2_T, F) ? hashgrid_ordered_layout(N, F).bytes : 0;
}

int sn_hashgrid_ordered_backward(const float* q, const float* table, const float* scalings, const float* grad_enc, int64_t N, int32_t L,
                                 int32_t log2_T, int32_t F, float* grad_table, float* grad_q, void* workspace, size_t workspace_bytes,
                                 SnStream stream) {
    return hashgrid_ordered_backward<HgOrderedEmit, HgInput>("sn_hashgrid_ordered_backward", q, table, scalings, grad_enc, N, L, log2_T, F, grad_table,
                                                             grad_q, workspace, workspace_bytes, stream);
}

int sn_hashgrid_ordered_tcnn_backward(const float* q, const float* table, const float* scalings, const float* grad_enc, int64_t N, int32_t L,
                                      int32_t log2_T, int32_t F, float* grad_table, float* grad_q, void* workspace, size_t workspace_bytes,
                                      SnStream stream) {
    return hashgrid_ordered_backward<HgOrderedEmitTcnn, HgTcnnInput>("sn_hashgrid_ordered_tcnn_backward", q, table, scalings, grad_enc, N, L, log2_T, F,
                                                                     grad_table, grad_q, workspace, workspace_bytes, stream);
}

}  // extern "C"
