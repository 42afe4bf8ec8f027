// sn_api_rays.h (part of sn_api.hip) -- camera rays, ray batches and box intersections (include/signerf_hip.h, signerf_hip_ray_batch.h)
#pragma once

extern "C" {

int sn_generate_rays_camera(const SnCameraDesc* cam, const float* coords, int64_t n_coords, float* origins, float* directions,
                            float* pixel_area, float* directions_norm, const float* aabb, float* nears, float* fars, SnStream stream) {
    if (!cam || cam->height <= 0 || cam->width <= 0 || (coords && n_coords < 0))
        return fail(nullptr, SN_ERR_INVALID, "sn_generate_rays_camera: bad argument");
    if (cam->camera_type != SN_CAMERA_PERSPECTIVE && cam->camera_type != SN_CAMERA_FISHEYE && cam->camera_type != SN_CAMERA_EQUIRECTANGULAR)
        return fail(nullptr, SN_ERR_INVALID, "sn_generate_rays_camera: camera_type " + std::to_string(cam->camera_type) +
                                                 " is not supported (1 = PERSPECTIVE, 2 = FISHEYE, 3 = EQUIRECTANGULAR)");
    SnRayGenParams p;
    memset(&p, 0, sizeof(p));
    memcpy(p.c2w, cam->c2w, sizeof(p.c2w));
    p.fx = cam->fx;
    p.fy = cam->fy;
    p.cx = cam->cx;
    p.cy = cam->cy;
    p.height = cam->height;
    p.width = cam->width;
    p.camera_type = cam->camera_type;
    p.has_distortion = cam->has_distortion != 0 && cam->camera_type != SN_CAMERA_EQUIRECTANGULAR;  // (nerfstudio never un-distorts equirectangular images)
    memcpy(p.dist, cam->distortion, sizeof(p.dist));
    p.coords = coords;
    p.n = coords ? n_coords : (int64_t)cam->height * cam->width;
    p.origins = origins;
    p.directions = directions;
    p.pixel_area = pixel_area;
    p.directions_norm = directions_norm;
    p.has_aabb = aabb != nullptr;
    if (aabb) memcpy(p.aabb, aabb, sizeof(p.aabb));
    p.nears = nears;
    p.fars = fars;
    if (p.n == 0) return SN_OK;
    void (*kernel)(SnRayGenParams) = p.has_distortion ? sn_generate_rays_kernel<1, true> : sn_generate_rays_kernel<1, false>;
    if (cam->camera_type == SN_CAMERA_EQUIRECTANGULAR) kernel = sn_generate_rays_kernel<3, false>;
    if (cam->camera_type == SN_CAMERA_FISHEYE) kernel = p.has_distortion ? sn_generate_rays_kernel<2, true> : sn_generate_rays_kernel<2, false>;
    hipLaunchKernelGGL(kernel, blocks_for(p.n), dim3(256), 0, (hipStream_t)stream, p);
    return end_launches("sn_generate_rays");
}

int sn_generate_rays(const float* c2w, float fx, float fy, float cx, float cy, int32_t height, int32_t width, float* origins,
                     float* directions, float* pixel_area, float* directions_norm, const float* aabb, float* nears, float* fars,
                     SnStream stream) {
    if (!c2w || height <= 0 || width <= 0) return fail(nullptr, SN_ERR_INVALID, "sn_generate_rays: bad argument");
    SnCameraDesc cam;
    memset(&cam, 0, sizeof(cam));
    memcpy(cam.c2w, c2w, sizeof(cam.c2w));
    cam.fx = fx;
    cam.fy = fy;
    cam.cx = cx;
    cam.cy = cy;
    cam.height = height;
    cam.width = width;
    cam.camera_type = SN_CAMERA_PERSPECTIVE;
    return sn_generate_rays_camera(&cam, nullptr, 0, origins, directions, pixel_area, directions_norm, aabb, nears, fars, stream);
}

int sn_intersect_with_aabb(const float* origins, const float* directions, int64_t n_rays, const float* aabb, float* nears,
                           float* fars, SnStream stream) {
    if (!origins || !directions || !aabb || !nears || !fars || n_rays < 0)
        return fail(nullptr, SN_ERR_INVALID, "sn_intersect_with_aabb: bad argument");
    if (n_rays == 0) return SN_OK;
    SnAabb box;
    memcpy(box.v, aabb, sizeof(box.v));
    hipLaunchKernelGGL(sn_intersect_with_aabb_kernel, blocks_for(n_rays), dim3(256), 0, (hipStream_t)stream, origins, directions, n_rays, box,
                       nears, fars);
    return end_launches("sn_intersect_with_aabb");
}

int sn_intersect_obb(const float* origins, const float* directions, int64_t n_rays, const float* world2box, const float* size,
                     float* nears, float* fars, SnStream stream) {
    if (!origins || !directions || !world2box || !size || !nears || !fars || n_rays < 0)
        return fail(nullptr, SN_ERR_INVALID, "sn_intersect_obb: bad argument");
    if (n_rays == 0) return SN_OK;
    SnObb box;
    memcpy(box.w2b, world2box, sizeof(box.w2b));
    for (int c = 0; c < 3; ++c) box.half[c] = size[c] / 2.0f;
    hipLaunchKernelGGL(sn_intersect_obb_kernel, blocks_for(n_rays), dim3(256), 0, (hipStream_t)stream, origins, directions, n_rays, box,
                       nears, fars);
    return end_launches("sn_intersect_obb");
}

// ---- include/signerf_hip_ray_batch.h: rays of many cameras in one launch ---------------------------------------------------------------
int sn_ray_batch_abi_version(void) { return SN_RAY_BATCH_ABI_VERSION; }

int sn_generate_ray_batch(const SnCameraDesc* cameras, int32_t n_cameras, const int64_t* ray_indices, const int64_t* camera_indices,
                          const float* coords, int64_t n, float* origins, float* directions, float* pixel_area, float* directions_norm,
                          const float* aabb, float* nears, float* fars, const uint8_t* images, int32_t img_h, int32_t img_w,
                          int32_t img_c, float* pixels, SnStream stream) {
    const std::string who = "sn_generate_ray_batch";
    if (!cameras || n_cameras < 1 || n < 0) return fail(nullptr, SN_ERR_INVALID, who + ": bad argument (cameras, n_cameras >= 1, n >= 0)");
    const bool triplets = ray_indices != nullptr, pairs = camera_indices != nullptr || coords != nullptr;
    if (triplets == pairs)
        return fail(nullptr, SN_ERR_INVALID, who + ": give exactly one index form, ray_indices [n,3] or camera_indices [n] with coords [n,2]");
    if (pairs && (!camera_indices || !coords)) return fail(nullptr, SN_ERR_INVALID, who + ": camera_indices and coords go together");
    if ((images != nullptr) != (pixels != nullptr)) return fail(nullptr, SN_ERR_INVALID, who + ": images and pixels go together");
    if (images) {
        if (!triplets) return fail(nullptr, SN_ERR_INVALID, who + ": pixels are gathered with the ray_indices form only");
        if (img_h < 1 || img_w < 1 || img_c < 1 || img_c > 4)
            return fail(nullptr, SN_ERR_INVALID, who + ": the image stack needs img_h, img_w >= 1 and img_c in 1..4");
    }
    if (n == 0) return SN_OK;
    SnRayBatchParams p;
    memset(&p, 0, sizeof(p));
    p.cameras = cameras;
    p.n_cameras = n_cameras;
    p.ray_indices = ray_indices;
    p.camera_indices = camera_indices;
    p.coords = coords;
    p.n = n;
    p.origins = origins;
    p.directions = directions;
    p.pixel_area = pixel_area;
    p.directions_norm = directions_norm;
    p.has_aabb = aabb != nullptr;
    if (aabb) memcpy(p.aabb, aabb, sizeof(p.aabb));
    p.nears = nears;
    p.fars = fars;
    p.images = images;
    p.img_h = img_h;
    p.img_w = img_w;
    p.img_c = img_c;
    p.pixels = pixels;
    if ((n + 255) / 256 > 0x7fffffffll) return fail(nullptr, SN_ERR_INVALID, who + ": n exceeds the grid (2^31 - 1 blocks of 256 rays)");
    hipLaunchKernelGGL(sn_ray_batch_kernel, blocks_for(n), dim3(256), 0, (hipStream_t)stream, p);
    return end_launches(who);
}

}  // extern "C"
