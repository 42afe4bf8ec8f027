// sn_api_mlp.h (part of sn_api.hip) -- include/signerf_hip_mlp.h: the trainable MLP on caller-owned weights
#pragma once

static_assert(SN_MLP_MAX_LAYERS == SN_MLP_LAYERS && SN_MLP_MAX_DIM == 16 * SN_MLP_TILES, "the header's limits are the kernels' tile counts");
static_assert(2 * SN_MLP_HALF_KBLOCKS == SN_MLP_TILES && offsetof(SnMlpDesc, precision) == 28, "precision sits in the slot `reserved` had");
static_assert(sizeof(SnMlpDesc) == 32 + 4 * SN_MLP_MAX_LAYERS * sizeof(void*), "SnMlpDesc has no padding the binding does not know");

namespace {

// the descriptor checks every entry point shares; fills the kernels' layer table
int check_mlp_desc(const std::string& who, const SnMlpDesc* d, SnMlpParams& p) {
    memset(&p, 0, sizeof(p));
    if (!d) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (desc)");
    if (d->struct_size != sizeof(SnMlpDesc))
        return fail(nullptr, SN_ERR_INVALID, who + ": SnMlpDesc.struct_size " + std::to_string(d->struct_size) + " is not a size this library knows (" +
                                                 std::to_string(sizeof(SnMlpDesc)) + ")");
    if (d->n_layers < 1 || d->n_layers > SN_MLP_MAX_LAYERS)
        return fail(nullptr, SN_ERR_INVALID, who + ": n_layers must lie in 1.." + std::to_string(SN_MLP_MAX_LAYERS));
    for (int i = 0; i <= d->n_layers; ++i)
        if (d->dims[i] < 1 || d->dims[i] > SN_MLP_MAX_DIM)
            return fail(nullptr, SN_ERR_INVALID, who + ": dims[" + std::to_string(i) + "] must lie in 1.." + std::to_string(SN_MLP_MAX_DIM));
    p.n_layers = d->n_layers;
    for (int i = 0; i <= d->n_layers; ++i) p.dims[i] = d->dims[i];
    for (int i = 0; i < d->n_layers; ++i) p.image += d->dims[i + 1] * d->dims[i] + d->dims[i + 1];
    return SN_OK;
}

// SnMlpDesc.precision (the field a library built before it existed ignored as `reserved`): one of the two arithmetics, or a refusal
int check_mlp_precision(const std::string& who, const SnMlpDesc* d) {
    if (d->precision != SN_MLP_PRECISION_FP32 && d->precision != SN_MLP_PRECISION_FP16)
        return fail(nullptr, SN_ERR_INVALID, who + ": SnMlpDesc.precision " + std::to_string(d->precision) + " is neither SN_MLP_PRECISION_FP32 (0) nor SN_MLP_PRECISION_FP16 (1)");
    return SN_OK;
}

int32_t mlp_partials(int64_t N) {
    return (int32_t)std::min<int64_t>((N + SN_MLP_WG_POINTS - 1) / SN_MLP_WG_POINTS, SN_MLP_MAX_PARTIALS);
}

// N and the pointers common to both passes; *launch says whether anything is left to do
int check_mlp_call(const std::string& who, const SnMlpDesc* d, int64_t N, bool pointers_ok, const char* pointers, SnMlpParams& p, bool* launch) {
    *launch = false;
    if (N < 0) return fail(nullptr, SN_ERR_INVALID, who + ": N must be >= 0");
    if (N > 0x7fffffffll) return fail(nullptr, SN_ERR_INVALID, who + ": N exceeds the grid (2^31 - 1 points)");
    if (N == 0) return SN_OK;
    if (!pointers_ok) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (" + pointers + ")");
    for (int i = 0; i < d->n_layers; ++i) {
        if (!d->weights[i] || !d->biases[i]) return fail(nullptr, SN_ERR_INVALID, who + ": NULL weights or biases of layer " + std::to_string(i));
        if (((uintptr_t)d->weights[i] | (uintptr_t)d->biases[i]) & 3)
            return fail(nullptr, SN_ERR_INVALID, who + ": weights and biases must be aligned to 4 bytes");
        p.W[i] = d->weights[i];
        p.b[i] = d->biases[i];
    }
    p.N = N;
    *launch = true;
    return SN_OK;
}

}  // namespace

extern "C" {

int sn_mlp_abi_version(void) { return SN_MLP_ABI_VERSION; }

int sn_mlp_forward(const SnMlpDesc* desc, const float* x, int64_t N, float* y, SnStream stream) {
    const std::string who = "sn_mlp_forward";
    SnMlpParams p;
    bool launch;
    if (int rc = check_mlp_desc(who, desc, p)) return rc;
    if (int rc = check_mlp_precision(who, desc)) return rc;
    if (int rc = check_mlp_call(who, desc, N, x && y, "x, y", p, &launch)) return rc;
    if (!launch) return SN_OK;
    if (((uintptr_t)x | (uintptr_t)y) & 3) return fail(nullptr, SN_ERR_INVALID, who + ": x and y must be aligned to 4 bytes");
    p.x = x;
    p.y = y;
    hipLaunchKernelGGL(desc->precision == SN_MLP_PRECISION_FP16 ? sn_train_mlp_half_forward_kernel : sn_train_mlp_forward_kernel,
                       blocks_for(N, SN_MLP_WG_POINTS), dim3(SN_MLP_BLOCK), 0, (hipStream_t)stream, p);
    return end_launches(who);
}

size_t sn_mlp_backward_workspace_bytes(const SnMlpDesc* desc, int64_t N) {
    SnMlpParams p;
    const std::string who = "sn_mlp_backward_workspace_bytes";
    if (check_mlp_desc(who, desc, p) != SN_OK || check_mlp_precision(who, desc) != SN_OK || N <= 0 || N > 0x7fffffffll) return 0;
    return (size_t)mlp_partials(N) * (size_t)p.image * sizeof(float);
}

int sn_mlp_backward(const SnMlpDesc* desc, const float* x, const float* grad_y, int64_t N, float* grad_x, void* workspace,
                    size_t workspace_bytes, SnStream stream) {
    const std::string who = "sn_mlp_backward";
    SnMlpParams p;
    bool launch;
    if (int rc = check_mlp_desc(who, desc, p)) return rc;
    if (int rc = check_mlp_precision(who, desc)) return rc;
    int n_grads = 0;
    for (int i = 0; i < desc->n_layers; ++i) n_grads += (desc->grad_weights[i] ? 1 : 0) + (desc->grad_biases[i] ? 1 : 0);
    if (n_grads != 0 && n_grads != 2 * desc->n_layers)
        return fail(nullptr, SN_ERR_INVALID, who + ": grad_weights and grad_biases must be set for every layer or for none");
    if (int rc = check_mlp_call(who, desc, N, x && grad_y && (grad_x || n_grads), "x, grad_y; grad_x or the weight gradients", p, &launch)) return rc;
    if (!launch) return SN_OK;
    if (((uintptr_t)x | (uintptr_t)grad_y | (uintptr_t)grad_x | (uintptr_t)workspace) & 3)
        return fail(nullptr, SN_ERR_INVALID, who + ": x, grad_y, grad_x and workspace must be aligned to 4 bytes");
    p.x = x;
    p.g = grad_y;
    p.dx = grad_x;
    p.n_partials = mlp_partials(N);
    if (n_grads) {
        const size_t need = (size_t)p.n_partials * (size_t)p.image * sizeof(float);
        if (!workspace || workspace_bytes < need)
            return fail(nullptr, SN_ERR_INVALID, who + ": workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) +
                                                     " needed (sn_mlp_backward_workspace_bytes)");
        for (int i = 0; i < desc->n_layers; ++i) {
            if (((uintptr_t)desc->grad_weights[i] | (uintptr_t)desc->grad_biases[i]) & 3)
                return fail(nullptr, SN_ERR_INVALID, who + ": grad_weights and grad_biases must be aligned to 4 bytes");
            p.dW[i] = desc->grad_weights[i];
            p.db[i] = desc->grad_biases[i];
        }
        p.partials = (float*)workspace;
    }
    hipLaunchKernelGGL(desc->precision == SN_MLP_PRECISION_FP16 ? sn_train_mlp_half_backward_kernel : sn_train_mlp_backward_kernel,
                       dim3((unsigned)p.n_partials), dim3(SN_MLP_BLOCK), 0, (hipStream_t)stream, p);
    if (n_grads) hipLaunchKernelGGL(sn_train_mlp_reduce_kernel, blocks_for(p.image, SN_MLP_BLOCK), dim3(SN_MLP_BLOCK), 0, (hipStream_t)stream, p);
    return end_launches(who);
}

}  // extern "C"
