/*
 * signerf_hip_mesh_color.h -- companion header of signerf_hip_mesh.h: the proxy mesh's colour image and the aabb masking mode's
 * combine_shape_with_depth condition (signerf/datasetgenerator/datasetgenerator.py:794-811).  The reference renders the mesh's colour with
 * pyrender in a scene lit by an ambient light only (signerf/renderer/renderer.py:64-196) and pastes channel 0 of it into the ControlNet
 * condition wherever the mesh is in front of the NeRF; these entry points do both on the device.  Exported from the same
 * libsignerf_hip.so and following the conventions of signerf_hip.h (int status, sn_last_error, caller-owned device memory and
 * workspace, work enqueued on the caller's stream, no hidden sync).
 *
 * Versioning: SN_MESH_COLOR_ABI_VERSION / sn_mesh_color_abi_version() version THIS header's signatures, as SN_MESH_ABI_VERSION does for
 * signerf_hip_mesh.h; SnMeshShadeOpts begins with struct_size like the versioned structs of signerf_hip.h ("ABI evolution" there).
 */
#ifndef SIGNERF_HIP_MESH_COLOR_H
#define SIGNERF_HIP_MESH_COLOR_H

#include "signerf_hip_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_MESH_COLOR_ABI_VERSION 1
int sn_mesh_color_abi_version(void);

/* The shading of a pyrender scene with an ambient light only: per covered pixel
 *   x = ambient * base_color.rgb * COLOR_0   (COLOR_0: the vertex colours / 255, interpolated perspective-correctly; 1 without them)
 *   x = pow(x, 1 / 2.2) if gamma,  colour = round(255 * clamp(x, 0, 1))
 * and round(255 * clamp(background, 0, 1)) where nothing covers the pixel centre.  base_color[3] (alpha) is carried and not used: the
 * image holds RGB only. */
typedef struct SnMeshShadeOpts {
    uint32_t struct_size;  /* sizeof(SnMeshShadeOpts) in the caller's header */
    float base_color[4];   /* material baseColorFactor, RGBA */
    float ambient[3];      /* the scene's ambient light */
    float background[3];   /* clear colour in [0, 1] */
    int32_t gamma;         /* != 0: the sRGB-like pow(x, 1 / 2.2) of pyrender's mesh shader */
} SnMeshShadeOpts;

/* Workspace of sn_mesh_raster_color: as sn_mesh_workspace_bytes (a function of the triangle count only); 0 for a bad argument. */
size_t sn_mesh_color_workspace_bytes(int64_t n_triangles, int32_t height, int32_t width);

/* Colour (and z-depth) image of a triangle mesh, sampled at pixel centres: the pixel grid, the coverage rule, the culling, the near / far
 * planes and every argument shared with sn_mesh_raster_depth as there.
 *   vertex_colors [n_vertices, 4] uint8 RGBA (device), or NULL for none.
 *   depth [height, width] fp32 (device) or NULL: when given, bit-identical to what sn_mesh_raster_depth writes for the same inputs.
 *   color [height, width, 3] uint8 (device): the front-most covering triangle's shaded colour (SnMeshShadeOpts); of two triangles at
 *   the same depth the one with the lower index wins (GL_LESS keeps the first drawn).  Deterministic: no atomics. */
int sn_mesh_raster_color(const float* vertices, int64_t n_vertices, const uint8_t* vertex_colors, const int32_t* triangles,
                         int64_t n_triangles, const float* model_view, float fx, float fy, float cx, float cy, int32_t height, int32_t width,
                         const SnMeshRasterOpts* opts, const SnMeshShadeOpts* shade, float* depth, uint8_t* color, void* workspace,
                         size_t workspace_bytes, SnStream stream);

/* sn_aabb_mask_condition with combine_shape_with_depth (datasetgenerator.py:758-818), workspace sized by sn_mask_workspace_bytes.
 *   The mask is sn_aabb_mask_condition's, bit for bit.  Where something is visible, condition [H,W,1] fp32 (may be NULL)
 *   = 1 - clamp(cv * mesh_color[..., 0] / 255 + !cv * nerf_norm, 0, 1) with cv = (mesh_depth < depth) & (mesh_depth > 0) (not inverted
 *   by inverse_mask) and nerf_norm the plain aabb condition's normalised depth.  Nothing visible: mask and condition all zeros.
 *   mesh_depth [H,W,1] fp32, mesh_color [H,W,3] uint8 (device), as sn_mesh_raster_color writes them. */
int sn_aabb_mask_condition_combined(const float* origins, const float* directions, const float* depth, int32_t height, int32_t width,
                                    const float* aabb, const SnMaskOpts* opts, const float* mesh_depth, const uint8_t* mesh_color,
                                    uint8_t* mask, float* condition, void* workspace, size_t workspace_bytes, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_MESH_COLOR_H */
