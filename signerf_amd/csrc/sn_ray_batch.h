// sn_ray_batch.h -- rays of many cameras in one launch (include/signerf_hip_ray_batch.h): ray i comes from camera c_i at the image
// coordinate (y_i, x_i).  One kernel, one lane per ray:
//   the lane loads its camera's SnCameraDesc record from the device table (104 bytes; a patch batch gives the 1024 consecutive rays of a
//   patch one record, a random batch gives every lane its own), switches on (camera_type, has_distortion) and calls sn_camera_ray
//   (sn_stage.h) -- the arithmetic of sn_generate_rays_kernel itself, so the result is that kernel's to the bit -- then, optionally,
//   gathers the uint8 pixel images[c, y, x, :] and writes it / 255.0f (IEEE division: torch's uint8.float() / 255).
// A camera index outside the table (or a record of an unsupported type) reads nothing further and writes NaN to every output of its ray;
// a (y, x) outside the image stack writes NaN pixels and a regular ray.  No LDS, no atomics.
#pragma once
#include "sn_device.h"
#include "sn_stage.h"

struct SnRayBatchParams {
    const SnCameraDesc* cameras;
    int n_cameras;
    const int64_t* ray_indices;     // [n,3] (camera, y, x), or nullptr: camera_indices + coords
    const int64_t* camera_indices;  // [n]
    const float* coords;            // [n,2] (y, x)
    int64_t n;
    float* origins;
    float* directions;
    float* pixel_area;
    float* directions_norm;
    int has_aabb;
    float aabb[6];
    float* nears;
    float* fars;
    const uint8_t* images;  // [n_cameras, img_h, img_w, img_c] or nullptr
    int img_h, img_w, img_c;
    float* pixels;          // [n, img_c]
};

__global__ __launch_bounds__(256) void sn_ray_batch_kernel(SnRayBatchParams p) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    int64_t c, iy = 0, ix = 0;
    float x, y;
    if (p.ray_indices) {
        c = p.ray_indices[i * 3 + 0];
        iy = p.ray_indices[i * 3 + 1];
        ix = p.ray_indices[i * 3 + 2];
        y = (float)iy + 0.5f;
        x = (float)ix + 0.5f;
    } else {
        c = p.camera_indices[i];
        y = p.coords[i * 2 + 0];
        x = p.coords[i * 2 + 1];
    }
    const bool box = p.has_aabb && p.nears && p.fars;
    const bool area = p.pixel_area != nullptr;
    bool ok = c >= 0 && c < (int64_t)p.n_cameras;
    SnRay r;
    if (ok) {
        const SnCameraDesc cam = p.cameras[c];
        const int type = cam.camera_type;
        const bool dist = cam.has_distortion != 0;
        if (type == SN_CAMERA_EQUIRECTANGULAR)  // (nerfstudio never un-distorts equirectangular images)
            sn_camera_ray<3, false>(cam.c2w, cam.fx, cam.fy, cam.cx, cam.cy, cam.distortion, x, y, area, box, p.aabb, r);
        else if (type == SN_CAMERA_FISHEYE && dist)
            sn_camera_ray<2, true>(cam.c2w, cam.fx, cam.fy, cam.cx, cam.cy, cam.distortion, x, y, area, box, p.aabb, r);
        else if (type == SN_CAMERA_FISHEYE)
            sn_camera_ray<2, false>(cam.c2w, cam.fx, cam.fy, cam.cx, cam.cy, cam.distortion, x, y, area, box, p.aabb, r);
        else if (type == SN_CAMERA_PERSPECTIVE && dist)
            sn_camera_ray<1, true>(cam.c2w, cam.fx, cam.fy, cam.cx, cam.cy, cam.distortion, x, y, area, box, p.aabb, r);
        else if (type == SN_CAMERA_PERSPECTIVE)
            sn_camera_ray<1, false>(cam.c2w, cam.fx, cam.fy, cam.cx, cam.cy, cam.distortion, x, y, area, box, p.aabb, r);
        else
            ok = false;
    }
    if (!ok) {
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < 3; ++k) r.o[k] = r.d[k] = nan;
        r.area = r.norm = r.tnear = r.tfar = nan;
    }
    sn_store_ray(r, i, p.origins, p.directions, p.pixel_area, p.directions_norm, box ? p.nears : nullptr, box ? p.fars : nullptr);
    if (p.pixels) {
        const bool in = ok && iy >= 0 && iy < (int64_t)p.img_h && ix >= 0 && ix < (int64_t)p.img_w;
        const uint8_t* src = p.images + (in ? ((c * p.img_h + iy) * p.img_w + ix) * p.img_c : 0);
        float* dst = p.pixels + i * p.img_c;
        for (int k = 0; k < p.img_c; ++k) dst[k] = in ? (float)src[k] / 255.0f : __builtin_nanf("");
    }
}
