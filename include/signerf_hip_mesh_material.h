/*
 * signerf_hip_mesh_material.h -- companion header of signerf_hip_mesh.h, signerf_hip_mesh_color.h and signerf_hip_mesh_rays.h: the proxy
 * mesh's colour image shaded with the mesh's own materials.  The reference loads its mesh with trimesh and draws it with pyrender, so an
 * OBJ that comes with an .mtl is drawn with its material: the Kd diffuse colour and, where there is one, the map_Kd texture.  The two
 * entry points here are sn_mesh_raster_color and sn_mesh_cast_rays with a set of materials in place of the vertex colours.  Exported
 * from the same libsignerf_hip.so and following the conventions of signerf_hip.h (int status, sn_last_error, caller-owned device memory
 * and workspace, work enqueued on the caller's stream, no hidden sync).
 *
 * Versioning: SN_MESH_MATERIAL_ABI_VERSION / sn_mesh_material_abi_version() version THIS header's signatures and the layout of
 * SnMeshMaterial; SnMeshMaterials begins with struct_size like the versioned structs of signerf_hip.h ("ABI evolution" there).
 */
#ifndef SIGNERF_HIP_MESH_MATERIAL_H
#define SIGNERF_HIP_MESH_MATERIAL_H

#include "signerf_hip_mesh_rays.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_MESH_MATERIAL_ABI_VERSION 1
int sn_mesh_material_abi_version(void);

/* One material, a frozen 32-byte record (the kernels read it from device memory).  tex_width = tex_height = 0: no texture (Kd only);
 * otherwise the texture is tex_width * tex_height RGBA8 texels (R first, alpha not used) from texel number texel_offset of the texel
 * blob, rows top to bottom as in the image file.  Two materials may share one texture. */
typedef struct SnMeshMaterial {
    float base_color[4];    /* Kd, alpha (carried and not used, as SnMeshShadeOpts.base_color[3]) */
    uint32_t texel_offset;  /* in texels (4 bytes each) from the start of the blob */
    int32_t tex_width, tex_height;
    uint32_t reserved;      /* 0 */
} SnMeshMaterial;

/* The materials of a mesh.  Per covered pixel, with b0..b2 the perspective-correct barycentrics of the drawn triangle's corners:
 *   uv  = b0 * uv0 + b1 * uv1 + b2 * uv2                    (the triangle's three per-CORNER texture coordinates)
 *   tex = bilinear(texture of the triangle's material, u, 1 - v): REPEAT wrap in both axes, texel centres at (i + 0.5) / size, the blend
 *         across the wrap seam takes the last and the first texel; the image's top row is v = 1.  1 when the material has no texture
 *         or corner_uv is NULL.  No mip maps.
 *   tex = pow(tex, 2.2) if texture_srgb
 *   x   = ambient * base_color.rgb * tex, then as SnMeshShadeOpts: pow(x, 1 / 2.2) if gamma, round(255 * clamp(x, 0, 1)).
 * What only the device can see gives a defined pixel and never a read outside the arrays: a triangle_material outside
 * [0, n_materials) is shaded with SnMeshShadeOpts.base_color (the default material) and tex = 1; a non-finite uv gives tex = 1; a
 * device record whose texture does not lie inside the blob is drawn as Kd only.
 *
 * The records live on the device, and the call reads nothing back: host_materials is the caller's HOST copy of the same n_materials
 * records, from which the call checks what it can before it launches anything (a side outside [1, 16384] where the other is not 0 too,
 * texel_offset + tex_width * tex_height beyond the blob, a base colour that is not finite: SN_ERR_INVALID). */
typedef struct SnMeshMaterials {
    uint32_t struct_size;                 /* sizeof(SnMeshMaterials) in the caller's header */
    int32_t n_materials;                  /* M in [1, 65535] */
    const SnMeshMaterial* materials;      /* [M] (device, 16-byte aligned) */
    const SnMeshMaterial* host_materials; /* [M] (host): the same records */
    const int32_t* triangle_material;     /* [n_triangles] (device): index into materials */
    const float* corner_uv;               /* [n_triangles, 3, 2] fp32 (device, 8-byte aligned), or NULL: no material's texture is drawn */
    const uint8_t* texels;                /* the RGBA8 texel blob (device, 4-byte aligned); may be NULL when texel_bytes is 0 */
    uint64_t texel_bytes;
    int32_t texture_srgb;                 /* != 0: the textures hold sRGB values, linearised with pow(., 2.2) */
    int32_t reserved;                     /* 0 */
} SnMeshMaterials;

/* sn_mesh_raster_color with `materials` in place of the vertex colours: every other argument, the workspace
 * (sn_mesh_color_workspace_bytes), the coverage rule and the tie rule as there; shade->base_color is the default material.
 *   depth (or NULL): bit-identical to what sn_mesh_raster_depth writes for the same inputs. */
int sn_mesh_raster_color_materials(const float* vertices, int64_t n_vertices, const SnMeshMaterials* materials, const int32_t* triangles,
                                   int64_t n_triangles, const float* model_view, float fx, float fy, float cx, float cy, int32_t height,
                                   int32_t width, const SnMeshRasterOpts* opts, const SnMeshShadeOpts* shade, float* depth, uint8_t* color,
                                   void* workspace, size_t workspace_bytes, SnStream stream);

/* sn_mesh_cast_rays with `materials` in place of the vertex colours.  color and shade are required (for the depth alone call
 * sn_mesh_cast_rays); triangles is not read (the uv are per corner) and may be NULL.
 *   depth: bit-identical to what sn_mesh_cast_rays writes for the same inputs. */
int sn_mesh_cast_rays_materials(const float* origins, const float* directions, int32_t height, int32_t width, const float* forward,
                                const void* accel, size_t accel_bytes, const int32_t* triangles, int64_t n_triangles,
                                const SnMeshMaterials* materials, int64_t n_vertices, const SnMeshRaysOpts* opts, const SnMeshShadeOpts* shade,
                                float* depth, uint8_t* color, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_MESH_MATERIAL_H */
