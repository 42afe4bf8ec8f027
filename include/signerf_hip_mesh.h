/*
 * signerf_hip_mesh.h -- companion header of signerf_hip.h: the "shape" masking mode of the dataset generator
 * (signerf/datasetgenerator/datasetgenerator.py:711-754).  The reference rasterises a proxy mesh's depth with pyrender on OpenGL / EGL
 * (signerf/renderer/renderer.py:64-196) and builds the mask and the ControlNet condition from it; these entry points do both on the
 * device.  Exported from the same libsignerf_hip.so and following the conventions of signerf_hip.h (int status, sn_last_error,
 * caller-owned device memory and workspace, work enqueued on the caller's stream, no hidden sync).
 *
 * Versioning: SN_MESH_ABI_VERSION / sn_mesh_abi_version() play the role SN_ABI_VERSION plays for the main header, for THIS header's
 * signatures; SnMeshRasterOpts begins with struct_size like the versioned structs of signerf_hip.h ("ABI evolution" there).
 */
#ifndef SIGNERF_HIP_MESH_H
#define SIGNERF_HIP_MESH_H

#include "signerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_MESH_ABI_VERSION 1
int sn_mesh_abi_version(void);

/* pyrender's IntrinsicsCamera(znear=1e-4, zfar=10) and its default (single-sided) material. */
typedef struct SnMeshRasterOpts {
    uint32_t struct_size;      /* sizeof(SnMeshRasterOpts) in the caller's header */
    float znear, zfar;         /* kept: znear <= z-depth <= zfar; 0 < znear < zfar */
    int32_t cull_back_faces;   /* != 0: GL_CULL_FACE / GL_BACK with counter-clockwise front faces */
} SnMeshRasterOpts;

/* Workspace of sn_mesh_raster_depth: 72 bytes per triangle (+ alignment); 0 for a bad argument. */
size_t sn_mesh_workspace_bytes(int64_t n_triangles, int32_t height, int32_t width);

/* z-depth image of a triangle mesh, sampled at pixel centres (pinhole; the pixel (i, j) samples the ray
 * ((j + 0.5 - cx) / fx, -(i + 0.5 - cy) / fy, -1) in OpenGL camera space -- the NeRF's pixel grid).
 *   vertices [n_vertices, 3] fp32, triangles [n_triangles, 3] int32 (device); an index outside [0, n_vertices) drops its triangle.
 *   model_view: 12 host floats, row-major 3x4 camera-from-object transform (OpenGL camera: x right, y up, looking down -z).
 *   depth [height, width] fp32 (device): the smallest z-depth in [znear, zfar] over the triangles that cover the pixel centre (a centre
 *   on an edge is inside), 0 where none does.  Deterministic: no atomics, bit-identical run to run.
 *   height, width in [1, 16384]; n_triangles in [0, 2^30] (0: all zeros). */
int sn_mesh_raster_depth(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const float* model_view,
                         float fx, float fy, float cx, float cy, int32_t height, int32_t width, const SnMeshRasterOpts* opts, float* depth,
                         void* workspace, size_t workspace_bytes, SnStream stream);

/* The shape-mode mask step (datasetgenerator.py:716-754), workspace sized by sn_mask_workspace_bytes(height, width).
 *   mesh_depth, nerf_depth [H,W,1] fp32 (device).  visible = (mesh_depth < nerf_depth) & (mesh_depth > 0), inverted with
 *   opts->inverse_mask.  mask [H,W,1] uint8 = visible dilated by the opts->dilate_w x dilate_h ellipse; condition [H,W,1] fp32 (may be NULL)
 *   = 1 - clamp(visible * obj_norm + !visible * nerf_norm, 0, 1), both depths normalised by [min - r, max + r] where min is taken over
 *   the visible pixels with mesh_depth > 0 and max over ALL mesh depths (or opts' manual range).  Nothing visible: mask and condition are
 *   all zeros.  Something visible but no visible pixel with mesh_depth > 0 (only with inverse_mask; the reference raises there): the mask
 *   as above, the condition all zeros. */
int sn_shape_mask_condition(const float* mesh_depth, const float* nerf_depth, int32_t height, int32_t width, const SnMaskOpts* opts,
                            uint8_t* mask, float* condition, void* workspace, size_t workspace_bytes, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_MESH_H */
