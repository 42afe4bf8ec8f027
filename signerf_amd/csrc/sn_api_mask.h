// sn_api_mask.h (part of sn_api.hip) -- the mask step in its three modes: aabb (include/signerf_hip.h), shape (signerf_hip_mesh.h) and
// aabb combined with the mesh's depth and colour (signerf_hip_mesh_color.h)
#pragma once

extern "C" size_t sn_mask_workspace_bytes(int32_t height, int32_t width) {
    if (height <= 0 || width <= 0) return 0;
    const size_t n = (size_t)height * width;
    return align256(n) + align256((size_t)height * (width + 1) * 4) + 256;
}

constexpr size_t kMaskOptsMin = offsetof(SnMaskOpts, additional_depth_radius) + sizeof(float);

// The part of SnMaskParams every masking mode shares: options (opts already adopted and validated), the elliptical element, the
// workspace carve-up (sn_mask_workspace_bytes) and the outputs.
static void fill_mask_params(const SnMaskOpts* opts, const float* depth, int32_t height, int32_t width, void* workspace, uint8_t* mask,
                             float* condition, SnMaskParams& p) {
    const size_t n = (size_t)height * width;
    memset(&p, 0, sizeof(p));
    p.depth = depth;
    p.height = height;
    p.width = width;
    p.inverse_mask = opts->inverse_mask;
    p.dilate = opts->dilate_w > 0;
    if (p.dilate) {
        // cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (w, h)): row i covers [c - dx, c + dx + 1) with
        // dx = round(c * sqrt((r*r - dy*dy) / (r*r))), r = h/2, c = w/2, dy = i - r (rows with |dy| > r are empty)
        const int kw = opts->dilate_w, kh = opts->dilate_h;
        const int r = kh / 2, c = kw / 2;
        const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
        p.el.kw = kw;
        p.el.kh = kh;
        p.el.ax = kw / 2;
        p.el.ay = kh / 2;
        for (int i = 0; i < kh; ++i) {
            int j1 = 0, j2 = 0;
            if (kw == 1 && kh == 1) j2 = 1;  // a 1x1 element is a rectangle
            else {
                const int dy = i - r;
                if (std::abs(dy) <= r) {
                    const int dx = (int)std::nearbyint(c * std::sqrt((r * r - dy * dy) * inv_r2));
                    j1 = std::max(c - dx, 0);
                    j2 = std::min(c + dx + 1, kw);
                }
            }
            p.el.j1[i] = (short)j1;
            p.el.j2[i] = (short)j2;
        }
    }
    p.has_manual_depth = opts->has_manual_depth;
    p.manual_min = (float)opts->manual_min;
    p.manual_range = (float)(opts->manual_max - opts->manual_min);
    p.depth_radius = opts->additional_depth_radius;
    char* ws = (char*)workspace;
    p.vis = (uint8_t*)ws;
    p.prefix = (int32_t*)(ws + align256(n));
    p.stats = (uint32_t*)(ws + align256(n) + align256((size_t)height * (width + 1) * 4));
    p.mask = mask;
    p.condition = condition;
}

// What the three mask entry points share, for the entry point `who`: adopt and validate SnMaskOpts, check the workspace and clear
// its stamp, fill p (fill_mask_params) and reset the three statistics words on the stream.
static int begin_mask_step(const std::string& who, const SnMaskOpts* opts, const float* depth, int32_t height, int32_t width, uint8_t* mask,
                           float* condition, void* workspace, size_t workspace_bytes, hipStream_t st, SnMaskParams& p) {
    SnMaskOpts o;
    if (int rc = adopt_struct(nullptr, opts, kMaskOptsMin, o, (who + ": SnMaskOpts").c_str())) return rc;
    if (o.dilate_w < 0 || o.dilate_h < 0 || o.dilate_w > SN_MASK_MAX_K || o.dilate_h > SN_MASK_MAX_K || ((o.dilate_w == 0) != (o.dilate_h == 0)))
        return fail(nullptr, SN_ERR_INVALID, who + ": dilation size must be 0 or within [1," + std::to_string(SN_MASK_MAX_K) + "] in both dimensions");
    if (!workspace || workspace_bytes < sn_mask_workspace_bytes(height, width)) return fail(nullptr, SN_ERR_WORKSPACE, who + ": workspace too small");
    clear_stamp(workspace);  // (a caller may hand the mask step the memory a render used: its bins are gone then)
    fill_mask_params(&o, depth, height, width, workspace, mask, condition, p);
    hipError_t e = hipMemsetAsync(p.stats, 0, 4, st);                    // count
    if (e == hipSuccess) e = hipMemsetAsync(p.stats + 1, 0xff, 4, st);  // ordered min
    if (e == hipSuccess) e = hipMemsetAsync(p.stats + 2, 0, 4, st);     // ordered max
    if (e != hipSuccess) return fail(nullptr, SN_ERR_HIP, who + " memset: " + hipGetErrorString(e));
    return SN_OK;
}

// the rays and the box of the two aabb modes
static void fill_mask_aabb(SnMaskParams& p, const float* origins, const float* directions, const float* aabb) {
    p.origins = origins;
    p.directions = directions;
    memcpy(p.aabb, aabb, sizeof(p.aabb));
}

// The launches of a mask step: the mode's visible-mask kernel over vp, the row prefix sums when dilating, the mode's condition kernel
// over cp; m is the SnMaskParams inside them.
template <typename V, typename Cn>
static int launch_mask_step(const std::string& who, void (*visible)(V), const V& vp, void (*condition)(Cn), const Cn& cp, const SnMaskParams& m,
                            hipStream_t st) {
    const int64_t n = (int64_t)m.height * m.width;
    hipLaunchKernelGGL(visible, dim3((unsigned)std::min<int64_t>((n + 255) / 256, SN_MASK_VIS_BLOCKS)), dim3(256), 0, st, vp);
    if (m.dilate) hipLaunchKernelGGL(sn_mask_prefix_kernel, dim3((unsigned)m.height), dim3(64), 0, st, m);
    hipLaunchKernelGGL(condition, blocks_for(n), dim3(256), 0, st, cp);
    return end_launches(who);
}

extern "C" {

int sn_aabb_mask_condition(const float* origins, const float* directions, const float* depth, int32_t height, int32_t width,
                           const float* aabb, const SnMaskOpts* opts, uint8_t* mask, float* condition, void* workspace,
                           size_t workspace_bytes, SnStream stream) {
    const std::string who = "sn_aabb_mask_condition";
    if (!origins || !directions || !depth || !aabb || !opts || !mask || height <= 0 || width <= 0)
        return fail(nullptr, SN_ERR_INVALID, who + ": bad argument");
    SnMaskParams p;
    if (int rc = begin_mask_step(who, opts, depth, height, width, mask, condition, workspace, workspace_bytes, (hipStream_t)stream, p)) return rc;
    fill_mask_aabb(p, origins, directions, aabb);
    return launch_mask_step(who, sn_mask_visible_kernel, p, sn_mask_condition_kernel, p, p, (hipStream_t)stream);
}

int sn_shape_mask_condition(const float* mesh_depth, const float* nerf_depth, int32_t height, int32_t width, const SnMaskOpts* opts,
                            uint8_t* mask, float* condition, void* workspace, size_t workspace_bytes, SnStream stream) {
    const std::string who = "sn_shape_mask_condition";
    if (!mesh_depth || !nerf_depth || !opts || !mask || height <= 0 || width <= 0)
        return fail(nullptr, SN_ERR_INVALID, who + ": bad argument");
    SnShapeMaskParams sp;
    if (int rc = begin_mask_step(who, opts, nerf_depth, height, width, mask, condition, workspace, workspace_bytes, (hipStream_t)stream, sp.m)) return rc;
    sp.mesh_depth = mesh_depth;
    return launch_mask_step(who, sn_shape_visible_kernel, sp, sn_shape_condition_kernel, sp, sp.m, (hipStream_t)stream);
}

int sn_aabb_mask_condition_combined(const float* origins, const float* directions, const float* depth, int32_t height, int32_t width,
                                    const float* aabb, const SnMaskOpts* opts, const float* mesh_depth, const uint8_t* mesh_color,
                                    uint8_t* mask, float* condition, void* workspace, size_t workspace_bytes, SnStream stream) {
    const std::string who = "sn_aabb_mask_condition_combined";
    if (!origins || !directions || !depth || !aabb || !opts || !mesh_depth || !mesh_color || !mask || height <= 0 || width <= 0)
        return fail(nullptr, SN_ERR_INVALID, who + ": bad argument");
    SnCombinedMaskParams cp;
    if (int rc = begin_mask_step(who, opts, depth, height, width, mask, condition, workspace, workspace_bytes, (hipStream_t)stream, cp.m)) return rc;
    fill_mask_aabb(cp.m, origins, directions, aabb);
    cp.mesh_depth = mesh_depth;
    cp.mesh_color = mesh_color;
    return launch_mask_step(who, sn_mask_visible_kernel, cp.m, sn_mask_condition_combined_kernel, cp, cp.m, (hipStream_t)stream);
}

}  // extern "C"
