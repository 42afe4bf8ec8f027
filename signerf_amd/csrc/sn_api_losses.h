// sn_api_losses.h (part of sn_api.hip) -- include/signerf_hip_losses.h: differentiable compositing and the sampler losses, one wave per ray
#pragma once

static_assert(SN_LOSSES_MAX_SAMPLES == SN_LOSS_MAX_S, "the header's sample limit is the kernels'");

// What every entry point does around its parameter block p (filling one reads no memory, so it is filled first): the checks, in this
// order; R == 0 is SN_OK with nothing launched (an empty tensor's pointer may be NULL); one wave per ray.
template <typename P>
static int launch_loss(const std::string& who, int64_t R, int32_t S, int32_t Pn, bool pointers_ok, const char* pointers, void (*kernel)(P), size_t lds_bytes,
                       const P& p, SnStream stream) {
    if (R < 0) return fail(nullptr, SN_ERR_INVALID, who + ": R must be >= 0");
    if (S < 1 || S > SN_LOSS_MAX_S) return fail(nullptr, SN_ERR_INVALID, who + ": S must lie in 1.." + std::to_string(SN_LOSS_MAX_S));
    if (Pn < 1 || Pn > SN_LOSS_MAX_S) return fail(nullptr, SN_ERR_INVALID, who + ": P must lie in 1.." + std::to_string(SN_LOSS_MAX_S));
    if (R == 0) return SN_OK;
    if (!pointers_ok) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (" + pointers + ")");
    if (R > 0x7fffffffll) return fail(nullptr, SN_ERR_INVALID, who + ": R exceeds the grid (2^31 - 1 rays)");
    hipLaunchKernelGGL(kernel, dim3((unsigned)R), dim3(64), lds_bytes, (hipStream_t)stream, p);
    return end_launches(who);
}

// The inputs a forward pass and its backward pass share; each adds its outputs, or its incoming and outgoing gradients.
static void fill_loss_inputs(SnLossCompositeParams& p, const float* deltas, const float* density, const float* colour, const float* background, int32_t S) {
    memset(&p, 0, sizeof(p));
    p.deltas = deltas;
    p.density = density;
    p.colour = colour;
    p.background = background;
    p.S = S;
}
static void fill_loss_inputs(SnLossDistortionParams& p, const float* t, const float* w, int32_t S) {
    memset(&p, 0, sizeof(p));
    p.t = t;
    p.w = w;
    p.S = S;
}
static void fill_loss_inputs(SnLossInterlevelParams& p, const float* t, const float* w, const float* t_env, const float* w_env, int32_t S, int32_t P) {
    memset(&p, 0, sizeof(p));
    p.t = t;
    p.w = w;
    p.t_env = t_env;
    p.w_env = w_env;
    p.S = S;
    p.P = P;
}

extern "C" {

int sn_losses_abi_version(void) { return SN_LOSSES_ABI_VERSION; }

int sn_loss_composite_forward(const float* deltas, const float* density, const float* colour, const float* background, int64_t R, int32_t S,
                              float* weights, float* rgb, float* accumulation, SnStream stream) {
    SnLossCompositeParams p;
    fill_loss_inputs(p, deltas, density, colour, background, S);
    p.weights = weights;
    p.rgb = rgb;
    p.accumulation = accumulation;
    return launch_loss("sn_loss_composite_forward", R, S, 1, deltas && density && (weights || rgb || accumulation) && (colour || !rgb),
                       "deltas, density; one output at least; colour with rgb", sn_loss_composite_forward_kernel, 0, p, stream);
}

int sn_loss_composite_backward(const float* deltas, const float* density, const float* colour, const float* background, int64_t R, int32_t S,
                               const float* grad_weights, const float* grad_rgb, const float* grad_acc, float* grad_density,
                               float* grad_colour, SnStream stream) {
    SnLossCompositeParams p;
    fill_loss_inputs(p, deltas, density, colour, background, S);
    p.grad_weights = grad_weights;
    p.grad_rgb = grad_rgb;
    p.grad_acc = grad_acc;
    p.grad_density = grad_density;
    p.grad_colour = grad_colour;
    return launch_loss("sn_loss_composite_backward", R, S, 1, deltas && density && grad_density && (colour || (!grad_rgb && !grad_colour)),
                       "deltas, density, grad_density; colour with grad_rgb or grad_colour", sn_loss_composite_backward_kernel, 0, p, stream);
}

int sn_loss_distortion_forward(const float* t, const float* w, int64_t R, int32_t S, float* loss, SnStream stream) {
    SnLossDistortionParams p;
    fill_loss_inputs(p, t, w, S);
    p.loss = loss;
    return launch_loss("sn_loss_distortion_forward", R, S, 1, t && w && loss, "t, w, loss", sn_loss_distortion_forward_kernel, sn_loss_distortion_lds(S), p,
                       stream);
}

int sn_loss_distortion_backward(const float* t, const float* w, const float* grad_loss, int64_t R, int32_t S, float* grad_w, SnStream stream) {
    SnLossDistortionParams p;
    fill_loss_inputs(p, t, w, S);
    p.grad_loss = grad_loss;
    p.grad_w = grad_w;
    return launch_loss("sn_loss_distortion_backward", R, S, 1, t && w && grad_loss && grad_w, "t, w, grad_loss, grad_w", sn_loss_distortion_backward_kernel,
                       sn_loss_distortion_lds(S), p, stream);
}

int sn_loss_interlevel_forward(const float* t, const float* w, const float* t_env, const float* w_env, int64_t R, int32_t S, int32_t P,
                               float* loss, float* w_outer, SnStream stream) {
    SnLossInterlevelParams p;
    fill_loss_inputs(p, t, w, t_env, w_env, S, P);
    p.loss = loss;
    p.w_outer = w_outer;
    return launch_loss("sn_loss_interlevel_forward", R, S, P, t && t_env && w_env && (loss || w_outer) && (w || !loss),
                       "t, t_env, w_env; loss or w_outer; w with loss", sn_loss_interlevel_forward_kernel, sn_loss_interlevel_lds(S, P, false), p, stream);
}

int sn_loss_interlevel_backward(const float* t, const float* w, const float* t_env, const float* w_env, const float* grad_loss, int64_t R,
                                int32_t S, int32_t P, float* grad_w_env, SnStream stream) {
    SnLossInterlevelParams p;
    fill_loss_inputs(p, t, w, t_env, w_env, S, P);
    p.grad_loss = grad_loss;
    p.grad_w_env = grad_w_env;
    return launch_loss("sn_loss_interlevel_backward", R, S, P, t && w && t_env && w_env && grad_loss && grad_w_env,
                       "t, w, t_env, w_env, grad_loss, grad_w_env", sn_loss_interlevel_backward_kernel, sn_loss_interlevel_lds(S, P, true), p, stream);
}

}  // extern "C"
