// sn_api_train_normals.h (part of sn_api.hip) -- include/signerf_hip_train_normals.h: analytic normals of training samples on the caller's
// hash table and nn.Linear stack.  Included after sn_api_hashgrid.h and sn_api_mlp.h: the checks are theirs.
#pragma once

namespace {

template <int F> struct TrainNormals { static constexpr void (*fn)(SnTrainNormalsParams) = sn_train_normals_analytic_kernel<F>; };

}  // namespace

extern "C" {

int sn_train_normals_abi_version(void) { return SN_TRAIN_NORMALS_ABI_VERSION; }

int sn_train_normals_analytic(const float* q, const float* table, const float* scalings, int64_t N, int32_t L, int32_t log2_T, int32_t F,
                              const SnMlpDesc* base_mlp, float* normals, float* grad_q, SnStream stream) {
    const std::string who = "sn_train_normals_analytic";
    SnMlpParams mp;
    bool launch;
    if (int rc = check_mlp_desc(who, base_mlp, mp)) return rc;
    if (int rc = check_hashgrid(who, N, L, log2_T, F, q && table && scalings && normals, "q, table, scalings, normals", {table}, nullptr, &launch)) return rc;
    if (base_mlp->dims[0] != L * F)
        return fail(nullptr, SN_ERR_INVALID, who + ": base_mlp->dims[0] = " + std::to_string(base_mlp->dims[0]) + " must equal L * F = " + std::to_string(L * F));
    if (!launch) return SN_OK;
    if (int rc = check_mlp_call(who, base_mlp, N, true, "", mp, &launch)) return rc;
    if (((uintptr_t)q | (uintptr_t)scalings | (uintptr_t)normals | (uintptr_t)grad_q) & 3)
        return fail(nullptr, SN_ERR_INVALID, who + ": q, scalings, normals and grad_q must be aligned to 4 bytes");
    SnTrainNormalsParams p;
    memset(&p, 0, sizeof(p));
    p.q = q;
    p.table = table;
    p.scal = scalings;
    p.normals = normals;
    p.grad_q = grad_q;
    p.N = N;
    p.L = L;
    p.log2_T = log2_T;
    p.n_layers = mp.n_layers;
    for (int i = 0; i <= mp.n_layers; ++i) p.dims[i] = mp.dims[i];
    for (int i = 0; i < mp.n_layers; ++i) {
        p.W[i] = mp.W[i];
        p.b[i] = mp.b[i];
    }
    hipLaunchKernelGGL(hashgrid_kernel_for<TrainNormals>(F), blocks_for(N, SN_MLP_WG_POINTS), dim3(SN_MLP_BLOCK), 0, (hipStream_t)stream, p);
    return end_launches(who);
}

}  // extern "C"
