// sn_mesh_material.h -- the proxy mesh's colour image shaded with the mesh's own MATERIALS (RendererConfig.materials = "mtl"): per
// triangle the .mtl material that `usemtl` assigned to it -- its Kd diffuse colour and, where it has one, its map_Kd texture, sampled at
// the triangle's per-corner texture coordinates.  What trimesh + pyrender draw for an OBJ that comes with an .mtl.  Two kernels, the
// sweep of sn_mesh_color.h (M-e) and the walk of sn_mesh_rays.h (M-r) with one epilogue in place of the vertex-colour one:
//   M-f  sn_mesh_tile_sweep<true> + sn_mesh_material_pixel
//   M-s  sn_mesh_rays_walk        + sn_mesh_material_pixel
// Per covered pixel, with b0..b2 the perspective-correct barycentrics of the winning triangle's corners:
//   uv  = b0 * uv0 + b1 * uv1 + b2 * uv2
//   tex = bilinear(texture, u, 1 - v): REPEAT in both axes, texel centres at (i + 0.5) / size, the blend across the wrap seam takes the
//         last and the first texel; 1 when the material has no texture (or the mesh no texture coordinates); pow(tex, 2.2) when
//         texture_srgb.  No mip maps.
//   x   = ambient * (Kd * tex), then the tail of sn_mesh_shade_pixel (sn_mesh_shade_channel, sn_unorm8), unchanged.
// The new loads per covered pixel: one 4-byte material index, the triangle's six uv floats (a 24-byte, 8-byte-aligned record read as
// three dwordx2), the 32-byte material record (two dwordx4; wave-mostly-uniform) and four 4-byte texels.  No atomics, no LDS of its
// own: bit-identical run to run.  The depth either kernel writes is what sn_mesh_tile_color_kernel / sn_mesh_rays_kernel write.
//
// Every index that reaches a load is tested first: a material index outside [0, M) shades with the default material (SnMeshShade.base)
// and texture value 1; a record whose texture does not fit the texel blob (or has a side outside [1, 16384]) is drawn without its
// texture; a non-finite uv gives texture value 1; the texel coordinates are wrapped into [0, size).
#pragma once
#include "sn_device.h"
#include "sn_mesh_color.h"
#include "sn_mesh_rays.h"

#define SN_MATERIAL_MAX_SIDE 16384

// = SnMeshMaterial of include/signerf_hip_mesh_material.h (32 bytes, 16-byte aligned on the device)
struct SnMeshMaterialRec {
    float base[4];        // Kd, alpha (carried, not used)
    uint32_t texel_offset;  // first texel of the texture in the blob, in texels
    int32_t tex_w, tex_h;   // 0: no texture
    uint32_t pad;
};
static_assert(sizeof(SnMeshMaterialRec) == 32, "material record layout");

struct SnMeshMaterialSet {
    const SnMeshMaterialRec* materials;  // [n_materials]
    const int32_t* triangle_material;    // [F]
    const float* corner_uv;              // [F,3,2] or NULL
    const uint32_t* texels;              // RGBA8, R in the low byte; rows top to bottom as in the image file
    uint64_t n_texels;
    int32_t n_materials;
    int32_t texture_srgb;
};

struct SnMeshMaterialColorParams {
    SnMeshRasterParams r;  // r.depth may be NULL
    SnMeshShade s;         // s.vertex_colors is not read; s.base = the default material
    SnMeshMaterialSet m;
    uint8_t* color;
};

struct SnMeshMaterialRaysParams {
    SnMeshRaysParams r;    // r.color is written; r.s as above
    SnMeshMaterialSet m;
};

// x in texel units (centre of texel i at i + 0.5), already reduced to [0, n]: the two texels the sample lies between, wrapped, and the
// weight of the second
SN_DEV void sn_material_axis(float x, int n, int& i0, int& i1, float& a) {
#pragma clang fp contract(off)
    const float c = x - 0.5f;
    const float fl = floorf(c);
    a = c - fl;
    i0 = (int)fl;  // in [-1, n]
    i0 = i0 < 0 ? i0 + n : i0;
    i0 = min(max(i0 >= n ? i0 - n : i0, 0), n - 1);
    i1 = i0 + 1 == n ? 0 : i0 + 1;
}

// One pixel's colour o[0..2]: the background for tri < 0, else triangle `tri` (< F: the caller's part) shaded with its material at the
// barycentric weights b0, b1, b2 of its corners.
SN_DEV void sn_mesh_material_pixel(const SnMeshShade& s, const SnMeshMaterialSet& m, int tri, float b0, float b1, float b2, uint8_t* o) {
    float rgb[3];
    if (tri < 0) {
        for (int c = 0; c < 3; ++c) rgb[c] = s.background[c];
    } else {
#pragma clang fp contract(off)
        float base[3] = {s.base[0], s.base[1], s.base[2]};
        float tex[3] = {1.0f, 1.0f, 1.0f};
        const int32_t mi = m.triangle_material[tri];
        if ((uint32_t)mi < (uint32_t)m.n_materials) {
            const f32x4* q = (const f32x4*)(m.materials + mi);
            const f32x4 q0 = q[0], q1 = q[1];
            base[0] = q0.x;
            base[1] = q0.y;
            base[2] = q0.z;
            const uint32_t off = __float_as_uint(q1.x);
            const int w = __float_as_int(q1.y), h = __float_as_int(q1.z);
            const bool fits = w >= 1 && h >= 1 && w <= SN_MATERIAL_MAX_SIDE && h <= SN_MATERIAL_MAX_SIDE &&
                              (uint64_t)off + (uint64_t)((uint32_t)w * (uint32_t)h) <= m.n_texels;
            if (m.corner_uv && fits) {
                const float2* uv = (const float2*)(m.corner_uv + (int64_t)tri * 6);
                const float2 t0 = uv[0], t1 = uv[1], t2 = uv[2];
                const float u = b0 * t0.x + b1 * t1.x + b2 * t2.x;
                const float v = b0 * t0.y + b1 * t1.y + b2 * t2.y;
                if (fabsf(u) < INFINITY && fabsf(v) < INFINITY) {  // (a NaN fails both)
                    const float vf = 1.0f - v;  // the image's top row is v = 1
                    int x0, x1, y0, y1;
                    float ax, ay;
                    sn_material_axis((u - floorf(u)) * (float)w, w, x0, x1, ax);
                    sn_material_axis((vf - floorf(vf)) * (float)h, h, y0, y1, ay);
                    const uint32_t* t = m.texels + off;
                    const uint32_t c00 = t[y0 * w + x0], c10 = t[y0 * w + x1], c01 = t[y1 * w + x0], c11 = t[y1 * w + x1];
                    for (int c = 0; c < 3; ++c) {
                        const float f00 = (float)((c00 >> (8 * c)) & 255u) / 255.0f, f10 = (float)((c10 >> (8 * c)) & 255u) / 255.0f;
                        const float f01 = (float)((c01 >> (8 * c)) & 255u) / 255.0f, f11 = (float)((c11 >> (8 * c)) & 255u) / 255.0f;
                        const float top = f00 + ax * (f10 - f00), bot = f01 + ax * (f11 - f01);
                        float x = top + ay * (bot - top);
                        if (m.texture_srgb) x = powf(fmaxf(x, 0.0f), 2.2f);
                        tex[c] = x;
                    }
                }
            }
        }
        for (int c = 0; c < 3; ++c) rgb[c] = sn_mesh_shade_channel(s.ambient[c], base[c], tex[c], s.gamma);
    }
    o[0] = sn_unorm8(rgb[0]);
    o[1] = sn_unorm8(rgb[1]);
    o[2] = sn_unorm8(rgb[2]);
}

// M-f
__global__ __launch_bounds__(SN_MESH_BATCH) void sn_mesh_tile_material_kernel(SnMeshMaterialColorParams cp) {
    const SnMeshRasterParams& p = cp.r;
    const SnMeshTileHit h = sn_mesh_tile_sweep<true>(p);
    if (!h.inside) return;
    const int64_t pix = (int64_t)h.py * p.width + h.px;
    if (p.depth) p.depth[pix] = h.z == INFINITY ? 0.0f : h.z;
    float b0 = 1.0f, b1 = 0.0f, b2 = 0.0f;
    if (h.tri >= 0) {
#pragma clang fp contract(off)
        const float s = h.e[0] + h.e[1] + h.e[2];  // (as in sn_mesh_tile_color_kernel)
        if (s != 0.0f) {
            b0 = h.e[0] / s;
            b1 = h.e[1] / s;
            b2 = h.e[2] / s;
        }
    }
    sn_mesh_material_pixel(cp.s, cp.m, h.tri, b0, b1, b2, cp.color + pix * 3);
}

// M-s
__global__ __launch_bounds__(SN_RAYS_BLOCK) void sn_mesh_rays_material_kernel(SnMeshMaterialRaysParams mp) {
    const SnMeshRaysParams& p = mp.r;
    int64_t ray;
    float f;
    SnRayHit h;
    if (!sn_mesh_rays_walk(p, ray, f, h)) return;
    const bool drawn = h.tri >= 0;
    p.depth[ray] = drawn ? h.t * f : 0.0f;
    const int tri = drawn && h.tri < p.n_tris ? h.tri : -1;  // (the blob's index: never read behind the per-triangle arrays)
    sn_mesh_material_pixel(p.s, mp.m, tri, 1.0f - h.u - h.v, h.u, h.v, p.color + ray * 3);
}
