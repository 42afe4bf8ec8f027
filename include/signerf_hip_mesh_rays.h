/*
 * signerf_hip_mesh_rays.h -- companion header of signerf_hip_mesh.h and signerf_hip_mesh_color.h: the proxy mesh's depth and colour
 * images for a camera that is not an ideal pinhole.  The two rasterisers draw the mesh through a pinhole, as the reference's pyrender
 * does, whatever lens the camera has; sn_mesh_cast_rays casts the camera's own per-pixel rays (what sn_generate_rays_camera wrote for it:
 * OPENCV distortion, FISHEYE, EQUIRECTANGULAR) against the mesh, so that the mesh image and the NeRF image it is compared with pixel by
 * pixel are the same projection.  Exported from the same libsignerf_hip.so and following the conventions of signerf_hip.h (int status,
 * sn_last_error, caller-owned device memory, work enqueued on the caller's stream, no hidden sync).
 *
 * Versioning: SN_MESH_RAYS_ABI_VERSION / sn_mesh_rays_abi_version() version THIS header's signatures and the layout of the acceleration
 * blob; SnMeshRaysOpts begins with struct_size like the versioned structs of signerf_hip.h ("ABI evolution" there).
 */
#ifndef SIGNERF_HIP_MESH_RAYS_H
#define SIGNERF_HIP_MESH_RAYS_H

#include "signerf_hip_mesh_color.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_MESH_RAYS_ABI_VERSION 1
int sn_mesh_rays_abi_version(void);

typedef struct SnMeshRaysOpts {
    uint32_t struct_size;      /* sizeof(SnMeshRaysOpts) in the caller's header */
    float znear, zfar;         /* drawn: znear < z-depth < zfar; 0 < znear < zfar */
    int32_t cull_back_faces;   /* != 0: only counter-clockwise (front) faces are drawn, as GL_CULL_FACE / GL_BACK */
} SnMeshRaysOpts;

/* Size of the acceleration blob of a mesh of n_triangles: a bounding-volume hierarchy over the POSED (world-space) triangles and a copy
 * of their corners.  The blob is built on the host (signerf_amd.renderer.build_accel), once per mesh and pose, and copied to the device;
 * its layout is private to the library version (it starts with a magic number and a version that the kernel checks: a blob of another
 * version, or of another triangle count, draws nothing).  0 for n_triangles outside [0, 2^26]. */
size_t sn_mesh_accel_bytes(int64_t n_triangles);

/* Depth (and colour) image of a triangle mesh along given rays: one ray per pixel, row-major.
 *   origins, directions [height * width, 3] fp32 (device), world space, as sn_generate_rays_camera writes them; directions need not be
 *   unit vectors.  forward: 3 host floats, the camera's viewing axis in world space (for a nerfstudio camera-to-world matrix: minus its
 *   third column); it is normalised here.
 *   accel: the blob (device, 16-byte aligned), accel_bytes = sn_mesh_accel_bytes(n_triangles).  The positions come from the blob.
 *   triangles [n_triangles, 3] int32 (device) and vertex_colors [n_vertices, 4] uint8 RGBA (device, or NULL) are read for the colour only:
 *   triangles may be NULL when color is NULL.
 *   depth [height, width] fp32 (device): z = t * (direction . forward) of the nearest DRAWN hit origin + t * direction, 0 where there is
 *   none -- the quantity sn_mesh_raster_depth writes.  Drawn: direction . forward > 0, znear < z < zfar and, with cull_back_faces, a
 *   front-facing triangle; a hit that is not drawn does not occlude (the rasteriser clips and culls before its depth test).  A ray that
 *   points backwards (direction . forward <= 0: the rear hemisphere of an EQUIRECTANGULAR camera, a FISHEYE beyond 180 degrees) draws
 *   nothing, as a frustum draws nothing behind its camera.
 *   color [height, width, 3] uint8 (device) or NULL: the hit triangle's colour, its vertex colours blended with the hit's barycentric
 *   weights and shaded as sn_mesh_raster_color shades (`shade`, required with color; the background where nothing is drawn).  Of two hits
 *   at the same distance the triangle with the lower index wins.  Deterministic: no atomics, bit-identical run to run.
 *   What differs from the rasterisers: no tile binning and no per-view triangle setup (the blob is per mesh); the nearest hit is chosen
 *   in fp32 ray distance; a ray on an edge is inside by the ray-triangle barycentrics (u, v >= 0, u + v <= 1), not by screen-space edge
 *   functions; the depth range is open.
 *   height, width in [1, 16384]. */
int sn_mesh_cast_rays(const float* origins, const float* directions, int32_t height, int32_t width, const float* forward,
                      const void* accel, size_t accel_bytes, const int32_t* triangles, int64_t n_triangles, const uint8_t* vertex_colors,
                      int64_t n_vertices, const SnMeshRaysOpts* opts, const SnMeshShadeOpts* shade, float* depth, uint8_t* color,
                      SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_MESH_RAYS_H */
