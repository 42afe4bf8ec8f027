/*
 * signerf_hip_ray_batch.h -- companion header of signerf_hip.h: rays of MANY cameras in one launch.  sn_generate_rays_camera serves one
 * camera per call; the reference's training data path (signerf/data/signerf_datamanager.py -> nerfstudio's RayGenerator ->
 * cameras.generate_rays(camera_indices=c[:, None], coords=...), fed by signerf/data/signerf_patch_pixel_sampler.py) draws every ray of a
 * batch from its own camera.  sn_generate_ray_batch takes (camera, y, x) per ray, looks the camera up in a device table and writes what
 * sn_generate_rays_camera writes for that camera and image coordinate -- to the bit: the two kernels share one copy of the arithmetic --
 * and, optionally, the matching pixel of an image stack.  Exported from the same libsignerf_hip.so and following the conventions of
 * signerf_hip.h (int status, sn_last_error, caller-owned device memory, work enqueued on the caller's stream, no hidden sync).
 *
 * Versioning: SN_RAY_BATCH_ABI_VERSION / sn_ray_batch_abi_version() version THIS header's signatures.  The camera record is
 * signerf_hip.h's SnCameraDesc (104 bytes, frozen by SN_ABI_VERSION).
 */
#ifndef SIGNERF_HIP_RAY_BATCH_H
#define SIGNERF_HIP_RAY_BATCH_H

#include "signerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_RAY_BATCH_ABI_VERSION 1
int sn_ray_batch_abi_version(void);

/* n rays, ray i from camera c_i at the image coordinate (y_i, x_i).
 *   cameras  DEVICE array of n_cameras SnCameraDesc records (n_cameras >= 1), filled as for sn_generate_rays_camera: has_distortion = 0
 *            skips the un-distortion, and an SN_CAMERA_EQUIRECTANGULAR record is never un-distorted.  The records' camera_type is read
 *            on the device: the CALLER checks on the host that every record holds a supported type (a ray of a record with another
 *            type is written as NaN, like a ray of a camera index outside the table).
 *   The indices come in exactly ONE of two forms (both, or neither: SN_ERR_INVALID):
 *     ray_indices     DEVICE int64 [n, 3] (camera, y, x): the image coordinate is the pixel centre (y + 0.5, x + 0.5) -- nerfstudio's
 *                     image_coords[y, x], what its RayGenerator passes;
 *     camera_indices  DEVICE int64 [n] together with coords DEVICE fp32 [n, 2] (y, x), as `generate_rays(camera_indices, coords)`.
 *   origins, directions [n, 3], pixel_area, directions_norm [n, 1]: DEVICE, any may be NULL.  aabb (6 HOST floats: min xyz, max xyz) or
 *   NULL; with it nears / fars [n, 1] (written when both are given) are nerfstudio's clamped slab test, 1e10 for a miss.
 *   images   optional DEVICE uint8 [n_cameras, img_h, img_w, img_c], img_c in 1..4, with pixels DEVICE fp32 [n, img_c] (both or neither;
 *            only with the ray_indices form): pixels[i, :] = images[c, y, x, :] / 255.0f, an IEEE division.
 * A camera index outside [0, n_cameras) reads nothing from the table: every float output of that ray, pixels included, is NaN.  A (y, x)
 * outside [0, img_h) x [0, img_w) gives NaN pixels; its ray is generated, since coordinates outside the image are legal for rays.
 * n == 0 returns SN_OK without a launch; n < 0, a NULL cameras, n_cameras < 1: SN_ERR_INVALID.  Deterministic: one lane per ray, no atomics. */
int sn_generate_ray_batch(const SnCameraDesc* cameras, int32_t n_cameras, const int64_t* ray_indices, const int64_t* camera_indices,
                          const float* coords, int64_t n, float* origins, float* directions, float* pixel_area, float* directions_norm,
                          const float* aabb, float* nears, float* fars, const uint8_t* images, int32_t img_h, int32_t img_w,
                          int32_t img_c, float* pixels, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_RAY_BATCH_H */
