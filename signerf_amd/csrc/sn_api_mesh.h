// sn_api_mesh.h (part of sn_api.hip) -- the proxy mesh: depth and colour rasters (include/signerf_hip_mesh.h, signerf_hip_mesh_color.h),
// the casts along the camera's own rays (signerf_hip_mesh_rays.h) and both with .mtl materials (signerf_hip_mesh_material.h)
#pragma once

#define SN_MESH_MAX_DIM 16384               // the tile records pack pixel coordinates into 16 bits
#define SN_MESH_MAX_TRIS ((int64_t)1 << 30)  // int32 triangle indexing in the kernels, with room for a batch past the end
#define SN_MESH_RAYS_MAX_TRIS ((int64_t)1 << 26)  // a leaf reference packs first * 8 + count into 31 bits

// The launches of a raster: M-a over the triangles (r, inside cp), then the entry point's tile kernel over cp
template <typename P>
static int launch_raster(const std::string& who, void (*tile_kernel)(P), const P& cp, const SnMeshRasterParams& r, hipStream_t st) {
    if (r.n_tris > 0) hipLaunchKernelGGL(sn_mesh_setup_kernel, blocks_for(r.n_tris), dim3(256), 0, st, r);
    const dim3 tiles((unsigned)((r.width + SN_MESH_TILE - 1) / SN_MESH_TILE), (unsigned)((r.height + SN_MESH_TILE - 1) / SN_MESH_TILE));
    hipLaunchKernelGGL(tile_kernel, tiles, dim3(SN_MESH_BATCH), 0, st, cp);
    return end_launches(who);
}

extern "C" {

int sn_mesh_abi_version(void) { return SN_MESH_ABI_VERSION; }
int sn_mesh_color_abi_version(void) { return SN_MESH_COLOR_ABI_VERSION; }
int sn_mesh_rays_abi_version(void) { return SN_MESH_RAYS_ABI_VERSION; }
int sn_mesh_material_abi_version(void) { return SN_MESH_MATERIAL_ABI_VERSION; }

size_t sn_mesh_workspace_bytes(int64_t n_triangles, int32_t height, int32_t width) {
    if (n_triangles < 0 || n_triangles > SN_MESH_MAX_TRIS || height <= 0 || width <= 0 || height > SN_MESH_MAX_DIM || width > SN_MESH_MAX_DIM)
        return 0;
    const size_t f = (size_t)n_triangles;
    return align256(f * sizeof(SnMeshTri)) + align256(f * sizeof(uint2)) + 256;
}

size_t sn_mesh_color_workspace_bytes(int64_t n_triangles, int32_t height, int32_t width) { return sn_mesh_workspace_bytes(n_triangles, height, width); }

size_t sn_mesh_accel_bytes(int64_t n_triangles) {
    if (n_triangles < 0 || n_triangles > SN_MESH_RAYS_MAX_TRIS) return 0;
    const size_t f = (size_t)n_triangles;
    return sizeof(SnMeshAccelHeader) + std::max<size_t>(f, 1) * sizeof(SnMeshAccelNode) + f * sizeof(SnMeshAccelTri);
}

// the first layouts
constexpr size_t kMeshRasterOptsMin = sizeof(SnMeshRasterOpts), kMeshShadeOptsMin = sizeof(SnMeshShadeOpts), kMeshRaysOptsMin = sizeof(SnMeshRaysOpts),
                 kMeshMaterialsMin = sizeof(SnMeshMaterials);
static_assert(sizeof(SnMeshMaterial) == sizeof(SnMeshMaterialRec), "the public record is the kernels' record");

// the depth range of SnMeshRasterOpts and SnMeshRaysOpts
static int check_depth_range(const std::string& who, float znear, float zfar) {
    if (!(znear > 0.0f) || !(zfar > znear) || !std::isfinite(zfar)) return fail(nullptr, SN_ERR_INVALID, who + ": need 0 < znear < zfar < inf");
    return SN_OK;
}

// SnMeshShadeOpts, adopted and checked for the entry point `who` -> the kernels' SnMeshShade
static int adopt_shade(const std::string& who, const SnMeshShadeOpts* shade, const uint8_t* vertex_colors, SnMeshShade& s) {
    SnMeshShadeOpts so;
    if (int rc = adopt_struct(nullptr, shade, kMeshShadeOptsMin, so, (who + ": SnMeshShadeOpts").c_str())) return rc;
    s.vertex_colors = vertex_colors;
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(so.base_color[c]) || !std::isfinite(so.ambient[c]) || !std::isfinite(so.background[c]))
            return fail(nullptr, SN_ERR_INVALID, who + ": base_color, ambient and background must be finite");
        s.base[c] = so.base_color[c];
        s.ambient[c] = so.ambient[c];
        s.background[c] = so.background[c];
    }
    s.gamma = so.gamma != 0;
    return SN_OK;
}

// What the three rasters share, for the entry point `who`: the checks of the mesh, the camera, SnMeshRasterOpts and the workspace (whose
// stamp is cleared), and the SnMeshRasterParams.  `outputs_ok`: the entry point's own required pointers are there.
static int begin_raster(const std::string& who, bool outputs_ok, const float* vertices, int64_t n_vertices, const int32_t* triangles,
                        int64_t n_triangles, const float* model_view, float fx, float fy, float cx, float cy, int32_t height, int32_t width,
                        const SnMeshRasterOpts* opts, float* depth, void* workspace, size_t workspace_bytes, SnMeshRasterParams& p) {
    if (!outputs_ok || !model_view || !opts || n_vertices < 0 || n_triangles < 0 || n_triangles > SN_MESH_MAX_TRIS || height <= 0 || width <= 0 ||
        height > SN_MESH_MAX_DIM || width > SN_MESH_MAX_DIM || (n_triangles > 0 && (!vertices || !triangles || n_vertices == 0)))
        return fail(nullptr, SN_ERR_INVALID, who + ": bad argument");
    SnMeshRasterOpts o;
    if (int rc = adopt_struct(nullptr, opts, kMeshRasterOptsMin, o, (who + ": SnMeshRasterOpts").c_str())) return rc;
    if (int rc = check_depth_range(who, o.znear, o.zfar)) return rc;
    if (!(fx != 0.0f) || !(fy != 0.0f) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail(nullptr, SN_ERR_INVALID, who + ": intrinsics must be finite with fx, fy != 0");
    if (!workspace || workspace_bytes < sn_mesh_workspace_bytes(n_triangles, height, width))
        return fail(nullptr, SN_ERR_WORKSPACE, who + ": workspace too small");
    clear_stamp(workspace);
    memset(&p, 0, sizeof(p));
    p.vertices = vertices;
    p.tris = triangles;
    p.n_vertices = n_vertices;
    p.n_tris = (int32_t)n_triangles;
    memcpy(p.mv, model_view, sizeof(p.mv));
    p.fx = fx;
    p.fy = fy;
    p.cx = cx;
    p.cy = cy;
    p.height = height;
    p.width = width;
    p.znear = o.znear;
    p.zfar = o.zfar;
    p.cull = o.cull_back_faces != 0;
    char* ws = (char*)workspace;
    p.rec = (SnMeshTri*)ws;
    p.bbox = (uint2*)(ws + align256((size_t)n_triangles * sizeof(SnMeshTri)));
    p.depth = depth;
    return SN_OK;
}

// What the two ray casts share, for the entry point `who`: the checks of the rays, the blob, SnMeshRaysOpts and (with a colour image)
// SnMeshShadeOpts, and the SnMeshRaysParams.
static int begin_cast_rays(const std::string& who, const float* origins, const float* directions, int32_t height, int32_t width,
                           const float* forward, const void* accel, size_t accel_bytes, const int32_t* triangles, int64_t n_triangles,
                           const uint8_t* vertex_colors, int64_t n_vertices, const SnMeshRaysOpts* opts, const SnMeshShadeOpts* shade,
                           float* depth, uint8_t* color, bool need_triangles, SnMeshRaysParams& p) {
    if (!origins || !directions || !forward || !accel || !opts || !depth || height <= 0 || width <= 0 || height > SN_MESH_MAX_DIM ||
        width > SN_MESH_MAX_DIM || n_triangles < 0 || n_triangles > SN_MESH_RAYS_MAX_TRIS || n_vertices < 0 ||
        (color && (!shade || (need_triangles && !triangles))))
        return fail(nullptr, SN_ERR_INVALID, who + ": bad argument");
    SnMeshRaysOpts o;
    if (int rc = adopt_struct(nullptr, opts, kMeshRaysOptsMin, o, (who + ": SnMeshRaysOpts").c_str())) return rc;
    if (int rc = check_depth_range(who, o.znear, o.zfar)) return rc;
    if (accel_bytes != sn_mesh_accel_bytes(n_triangles) || ((uintptr_t)accel & 15u) != 0)
        return fail(nullptr, SN_ERR_INVALID, who + ": accel must be a 16-byte-aligned blob of sn_mesh_accel_bytes(n_triangles) bytes");
    const double fn = std::sqrt((double)forward[0] * forward[0] + (double)forward[1] * forward[1] + (double)forward[2] * forward[2]);
    if (!std::isfinite(fn) || !(fn > 0.0)) return fail(nullptr, SN_ERR_INVALID, who + ": forward must be a finite non-zero vector");
    memset(&p, 0, sizeof(p));
    if (color)
        if (int rc = adopt_shade(who, shade, vertex_colors, p.s)) return rc;
    p.origins = origins;
    p.directions = directions;
    p.height = height;
    p.width = width;
    for (int k = 0; k < 3; ++k) p.fwd[k] = (float)(forward[k] / fn);
    p.znear = o.znear;
    p.zfar = o.zfar;
    p.cull = o.cull_back_faces != 0;
    p.accel = (const uint8_t*)accel;
    p.n_tris = (int32_t)n_triangles;
    p.tris = triangles;
    p.n_vertices = n_vertices;
    p.depth = depth;
    p.color = color;
    return SN_OK;
}

static dim3 cast_rays_grid(int32_t height, int32_t width) { return dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)); }
       
       // SnMeshMaterials (checked against its host copy of the records) -> the kernels' SnMeshMaterialSet
       static int adopt_materials(const std::string& who, const SnMeshMaterials* materials, int64_t n_triangles, SnMeshMaterialSet& m) {
    if (!materials) return fail(nullptr, SN_ERR_INVALID, who + ": materials is NULL");
    SnMeshMaterials a;
    if (int rc = adopt_struct(nullptr, materials, kMeshMaterialsMin, a, (who + ": SnMeshMaterials").c_str())) return rc;
    if (a.n_materials < 1 || a.n_materials > 65535) return fail(nullptr, SN_ERR_INVALID, who + ": n_materials must be in [1, 65535]");
    if (!a.materials || !a.host_materials || (n_triangles > 0 && !a.triangle_material))
        return fail(nullptr, SN_ERR_INVALID, who + ": materials, host_materials and triangle_material must not be NULL");
    if (((uintptr_t)a.materials & 15u) != 0 || ((uintptr_t)a.corner_uv & 7u) != 0 || ((uintptr_t)a.texels & 3u) != 0)
        return fail(nullptr, SN_ERR_INVALID, who + ": materials must be 16-byte, corner_uv 8-byte and texels 4-byte aligned");
    if (a.texel_bytes > 0 && !a.texels) return fail(nullptr, SN_ERR_INVALID, who + ": texels is NULL but texel_bytes is not 0");
    const uint64_t n_texels = a.texel_bytes / 4u;
    for (int32_t k = 0; k < a.n_materials; ++k) {
        const SnMeshMaterial& r = a.host_materials[k];
        const std::string which = who + ": material " + std::to_string(k);
        for (int c = 0; c < 4; ++c)
            if (!std::isfinite(r.base_color[c])) return fail(nullptr, SN_ERR_INVALID, which + ": base_color must be finite");
        if (r.tex_width == 0 && r.tex_height == 0) continue;
        if (r.tex_width < 1 || r.tex_height < 1 || r.tex_width > SN_MATERIAL_MAX_SIDE || r.tex_height > SN_MATERIAL_MAX_SIDE)
            return fail(nullptr, SN_ERR_INVALID, which + ": a texture side must be in [1, 16384] (or both 0: no texture)");
        if ((uint64_t)r.texel_offset + (uint64_t)r.tex_width * (uint64_t)r.tex_height > n_texels)
            return fail(nullptr, SN_ERR_INVALID, which + ": its texture ends beyond the texel blob (texel_bytes too small)");
    }
    m.materials = (const SnMeshMaterialRec*)a.materials;
    m.triangle_material = a.triangle_material;
    m.corner_uv = a.corner_uv;
    m.texels = (const uint32_t*)a.texels;
    m.n_texels = n_texels;
    m.n_materials = a.n_materials;
    m.texture_srgb = a.texture_srgb != 0;
    return SN_OK;
}

int sn_mesh_raster_depth(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const float* model_view,
                         float fx, float fy, float cx, float cy, int32_t height, int32_t width, const SnMeshRasterOpts* opts, float* depth,
                         void* workspace, size_t workspace_bytes, SnStream stream) {
    const std::string who = "sn_mesh_raster_depth";
    SnMeshRasterParams p;
    if (int rc = begin_raster(who, depth != nullptr, vertices, n_vertices, triangles, n_triangles, model_view, fx, fy, cx, cy, height, width, opts,
                              depth, workspace, workspace_bytes, p))
        return rc;
    return launch_raster(who, sn_mesh_tile_kernel, p, p, (hipStream_t)stream);
}

int sn_mesh_raster_color(const float* vertices, int64_t n_vertices, const uint8_t* vertex_colors, const int32_t* triangles,
                         int64_t n_triangles, const float* model_view, float fx, float fy, float cx, float cy, int32_t height, int32_t width,
                         const SnMeshRasterOpts* opts, const SnMeshShadeOpts* shade, float* depth, uint8_t* color, void* workspace,
                         size_t workspace_bytes, SnStream stream) {
    const std::string who = "sn_mesh_raster_color";
    SnMeshColorParams cp;
    memset(&cp, 0, sizeof(cp));
    if (int rc = begin_raster(who, shade && color, vertices, n_vertices, triangles, n_triangles, model_view, fx, fy, cx, cy, height, width, opts,
                              depth, workspace, workspace_bytes, cp.r))
        return rc;
    if (int rc = adopt_shade(who, shade, vertex_colors, cp.s)) return rc;
    cp.color = color;
    return launch_raster(who, sn_mesh_tile_color_kernel, cp, cp.r, (hipStream_t)stream);
}

int sn_mesh_raster_color_materials(const float* vertices, int64_t n_vertices, const SnMeshMaterials* materials, const int32_t* triangles,
                                   int64_t n_triangles, const float* model_view, float fx, float fy, float cx, float cy, int32_t height,
                                   int32_t width, const SnMeshRasterOpts* opts, const SnMeshShadeOpts* shade, float* depth, uint8_t* color,
                                   void* workspace, size_t workspace_bytes, SnStream stream) {
    const std::string who = "sn_mesh_raster_color_materials";
    SnMeshMaterialColorParams cp;
    memset(&cp, 0, sizeof(cp));
    if (n_triangles < 0) return fail(nullptr, SN_ERR_INVALID, who + ": bad argument");
    if (int rc = adopt_materials(who, materials, n_triangles, cp.m)) return rc;
    if (!shade) return fail(nullptr, SN_ERR_INVALID, who + ": bad argument");
    if (int rc = adopt_shade(who, shade, nullptr, cp.s)) return rc;
    if (int rc = begin_raster(who, color != nullptr, vertices, n_vertices, triangles, n_triangles, model_view, fx, fy, cx, cy, height, width, opts,
                              depth, workspace, workspace_bytes, cp.r))
        return rc;
    cp.color = color;
    return launch_raster(who, sn_mesh_tile_material_kernel, cp, cp.r, (hipStream_t)stream);
}

int sn_mesh_cast_rays(const float* origins, const float* directions, int32_t height, int32_t width, const float* forward,
                      const void* accel, size_t accel_bytes, const int32_t* triangles, int64_t n_triangles, const uint8_t* vertex_colors,
                      int64_t n_vertices, const SnMeshRaysOpts* opts, const SnMeshShadeOpts* shade, float* depth, uint8_t* color,
                      SnStream stream) {
    const std::string who = "sn_mesh_cast_rays";
    SnMeshRaysParams p;
    if (int rc = begin_cast_rays(who, origins, directions, height, width, forward, accel, accel_bytes, triangles, n_triangles, vertex_colors,
                                 n_vertices, opts, shade, depth, color, true, p))
        return rc;
    void (*kernel)(SnMeshRaysParams) = color ? sn_mesh_rays_kernel<true> : sn_mesh_rays_kernel<false>;
    hipLaunchKernelGGL(kernel, cast_rays_grid(height, width), dim3(SN_RAYS_BLOCK), 0, (hipStream_t)stream, p);
    return end_launches(who);
}

int sn_mesh_cast_rays_materials(const float* origins, const float* directions, int32_t height, int32_t width, const float* forward,
                                const void* accel, size_t accel_bytes, const int32_t* triangles, int64_t n_triangles,
                                const SnMeshMaterials* materials, int64_t n_vertices, const SnMeshRaysOpts* opts, const SnMeshShadeOpts* shade,
                                float* depth, uint8_t* color, SnStream stream) {
    const std::string who = "sn_mesh_cast_rays_materials";
    SnMeshMaterialRaysParams mp;
    memset(&mp, 0, sizeof(mp));
    if (!color || !shade || n_triangles < 0) return fail(nullptr, SN_ERR_INVALID, who + ": bad argument");
    if (int rc = adopt_materials(who, materials, n_triangles, mp.m)) return rc;
    if (int rc = begin_cast_rays(who, origins, directions, height, width, forward, accel, accel_bytes, triangles, n_triangles, nullptr, n_vertices,
                                 opts, shade, depth, color, false, mp.r))
        return rc;
    hipLaunchKernelGGL(sn_mesh_rays_material_kernel, cast_rays_grid(height, width), dim3(SN_RAYS_BLOCK), 0, (hipStream_t)stream, mp);
    return end_launches(who);
}

}  // extern "C"
