// sn_normal_losses.h -- the per-ray normal terms of a training step (include/signerf_hip_normal_losses.h), an extension of sn_losses.h's
// family: nerfstudio's orientation_loss and pred_normal_loss [NS-RECALL, model_components/losses.py] and the NormalsRenderer +
// NormalsShader pair (oracle.nerfacto.render_normals) in ONE pass over a ray's samples, and the gradient of the pred-normal term in the
// predicted normals -- the only gradient nerfacto's call needs (weights and analytic normals are detached there; the orientation term
// reads constants only).  The formulas are restated in DESIGN.md §4 "Training-mode normals"; tests/train_normals_oracle.py holds them as
// torch ops.
//
// Mapping and arithmetic: sn_losses.h's.  One wave per ray (64-thread blocks, block r is ray r), lane l takes the samples l, l + 64, ...;
// the inputs are fp32, every product and sum is fp64, the reductions are the fixed butterfly, each output is rounded to fp32 once.  No
// atomics, no LDS.
#pragma once
#include "sn_losses.h"

#define SN_NORMALS_RENDER_EPS 1e-10   // NormalsRenderer: v / (|v| + eps)

struct SnLossNormalsParams {
    const float* weights;        // [R,S]
    const float* normals;        // [R,S,3]
    const float* pred_normals;   // [R,S,3] or nullptr
    const float* directions;     // [R,3] or nullptr
    const float* grad_pred;      // [R]  (backward)
    int S;
    // forward, each may be nullptr
    float* orientation;     // [R]
    float* pred_normal;     // [R]
    float* rendered;        // [R,3]
    float* rendered_pred;   // [R,3]
    // backward
    float* grad_pred_normals;   // [R,S,3]
};

SN_DEV void sn_loss_shade_normal(const double (&v)[3], float* out) {   // (v / (|v| + eps) + 1) / 2
    const double norm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + SN_NORMALS_RENDER_EPS;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (float)((v[k] / norm + 1.0) * 0.5);
}

__global__ __launch_bounds__(64) void sn_loss_normals_forward_kernel(SnLossNormalsParams p) {
    const int lane = threadIdx.x, S = p.S;
    const int64_t row = (int64_t)blockIdx.x * S;
    const float* w = p.weights + row;
    const float* nr = p.normals + row * 3;
    const float* pr = p.pred_normals ? p.pred_normals + row * 3 : nullptr;
    double view[3] = {0.0, 0.0, 0.0};   // the view direction: minus the ray's
    if (p.directions) {
#pragma unroll
        for (int k = 0; k < 3; ++k) view[k] = -(double)p.directions[(int64_t)blockIdx.x * 3 + k];
    }
    double orient = 0.0, pred = 0.0, vn[3] = {0.0, 0.0, 0.0}, vp[3] = {0.0, 0.0, 0.0};
    for (int i = lane; i < S; i += 64) {
        const double wi = (double)w[i];
        const double n[3] = {(double)nr[i * 3], (double)nr[i * 3 + 1], (double)nr[i * 3 + 2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) vn[k] += wi * n[k];
        if (p.directions) {
            const double dot = n[0] * view[0] + n[1] * view[1] + n[2] * view[2];
            const double m = dot < 0.0 ? dot : 0.0;   // torch.fmin(0, dot): a NaN fails the comparison and gives 0
            orient += wi * (m * m);
        }
        if (pr) {
            const double q[3] = {(double)pr[i * 3], (double)pr[i * 3 + 1], (double)pr[i * 3 + 2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) vp[k] += wi * q[k];
            pred += wi * (1.0 - (n[0] * q[0] + n[1] * q[1] + n[2] * q[2]));
        }
    }
    // (the conditions below are kernel arguments: every lane of the wave reaches the same shuffles)
    if (p.orientation) orient = sn_loss_wave_sum(orient);
    if (p.pred_normal) pred = sn_loss_wave_sum(pred);
    if (p.rendered) {
#pragma unroll
        for (int k = 0; k < 3; ++k) vn[k] = sn_loss_wave_sum(vn[k]);
    }
    if (p.rendered_pred) {
#pragma unroll
        for (int k = 0; k < 3; ++k) vp[k] = sn_loss_wave_sum(vp[k]);
    }
    if (lane != 0) return;
    if (p.orientation) p.orientation[blockIdx.x] = (float)orient;
    if (p.pred_normal) p.pred_normal[blockIdx.x] = (float)pred;
    if (p.rendered) sn_loss_shade_normal(vn, p.rendered + (int64_t)blockIdx.x * 3);
    if (p.rendered_pred) sn_loss_shade_normal(vp, p.rendered_pred + (int64_t)blockIdx.x * 3);
}

// grad_pred_normals[s, :] = g w_s (-n_s)
__global__ __launch_bounds__(64) void sn_loss_normals_backward_kernel(SnLossNormalsParams p) {
    const int lane = threadIdx.x, S = p.S;
    const int64_t row = (int64_t)blockIdx.x * S;
    const double g = (double)p.grad_pred[blockIdx.x];
    for (int i = lane; i < S; i += 64) {
        const double gw = g * (double)p.weights[row + i];
#pragma unroll
        for (int k = 0; k < 3; ++k) p.grad_pred_normals[(row + i) * 3 + k] = (float)(gw * -(double)p.normals[(row + i) * 3 + k]);
    }
}
