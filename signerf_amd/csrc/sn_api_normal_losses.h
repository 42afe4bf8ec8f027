// sn_api_normal_losses.h (part of sn_api.hip) -- include/signerf_hip_normal_losses.h: the per-ray normal terms, one wave per ray.  Included
// after sn_api_losses.h: the checks and the launch are its launch_loss.
#pragma once

static void fill_loss_inputs(SnLossNormalsParams& p, const float* weights, const float* normals, int32_t S) {
    memset(&p, 0, sizeof(p));
    p.weights = weights;
    p.normals = normals;
    p.S = S;
}

extern "C" {

int sn_normal_losses_abi_version(void) { return SN_NORMAL_LOSSES_ABI_VERSION; }

int sn_loss_normals_forward(const float* weights, const float* normals, const float* pred_normals, const float* directions, int64_t R,
                            int32_t S, float* orientation, float* pred_normal, float* rendered_normals, float* rendered_pred_normals,
                            SnStream stream) {
    SnLossNormalsParams p;
    fill_loss_inputs(p, weights, normals, S);
    p.pred_normals = pred_normals;
    p.directions = directions;
    p.orientation = orientation;
    p.pred_normal = pred_normal;
    p.rendered = rendered_normals;
    p.rendered_pred = rendered_pred_normals;
    return launch_loss("sn_loss_normals_forward", R, S, 1,
                       weights && normals && (orientation || pred_normal || rendered_normals || rendered_pred_normals) &&
                           (pred_normals || (!pred_normal && !rendered_pred_normals)) && (directions || !orientation),
                       "weights, normals; one output at least; pred_normals with pred_normal or rendered_pred_normals; directions with orientation",
                       sn_loss_normals_forward_kernel, 0, p, stream);
}

int sn_loss_normals_backward(const float* weights, const float* normals, const float* grad_pred_normal, int64_t R, int32_t S,
                             float* grad_pred_normals, SnStream stream) {
    SnLossNormalsParams p;
    fill_loss_inputs(p, weights, normals, S);
    p.grad_pred = grad_pred_normal;
    p.grad_pred_normals = grad_pred_normals;
    return launch_loss("sn_loss_normals_backward", R, S, 1, weights && normals && grad_pred_normal && grad_pred_normals,
                       "weights, normals, grad_pred_normal, grad_pred_normals", sn_loss_normals_backward_kernel, 0, p, stream);
}

}  // extern "C"
