// sn_mesh_color.h -- the proxy mesh's COLOUR image and the aabb mode's combine_shape_with_depth condition
// (signerf/datasetgenerator/datasetgenerator.py:794-811, signerf/renderer/renderer.py:64-196 of the reference).  The reference renders the
// mesh with pyrender in a scene lit by an ambient light of 1 only and pastes channel 0 of the colour image into the ControlNet condition
// wherever the mesh is in front of the NeRF.  Here:
//   M-a  sn_mesh_setup_kernel of sn_mesh.h
//   M-e  per-tile colour + depth: sn_mesh_tile_sweep<true> of sn_mesh.h, which keeps besides the nearest depth the winning triangle (the
//        lowest index on a tie) and its three edge values e0..e2 -- normalised by their sum, the ray's perspective-correct barycentrics.
//        Per-pixel epilogue: interpolated vertex colour x base colour x ambient, optional gamma 1/2.2, unorm8; background where nothing
//        covers the centre.
//   K-a, K-b of sn_mask.h, then
//   K-d  K-c's mask (the same helpers), and the condition 1 - clamp(cv * colour[0] / 255 + !cv * nerf_norm, 0, 1),
//        cv = (mesh_depth < depth) & (mesh_depth > 0)
// No atomics in M-e (bit-identical run to run); M-e and M-b run one sweep, so they write one depth.
#pragma once
#include "sn_device.h"
#include "sn_mask.h"
#include "sn_mesh.h"

// The shading both mesh kernels share (this header's M-e and the ray cast of sn_mesh_rays.h).
struct SnMeshShade {
    const uint8_t* vertex_colors; // [V,4] RGBA8, or NULL (COLOR_0 = 1)
    float base[3];                // material baseColorFactor.rgb
    float ambient[3];
    float background[3];          // in [0, 1], written without gamma
    int gamma;                    // != 0: pow(x, 1 / 2.2) before the quantisation
};

struct SnMeshColorParams {
    SnMeshRasterParams r;         // r.depth may be NULL here
    SnMeshShade s;
    uint8_t* color;               // [H,W,3] out
};

SN_DEV uint8_t sn_unorm8(float x) {
#pragma clang fp contract(off)
    x = fminf(fmaxf(x, 0.0f), 1.0f);  // (also maps a NaN to 0)
    return (uint8_t)(int)(x * 255.0f + 0.5f);
}

// The tail every shading shares (vertex colours here, materials in sn_mesh_material.h): one channel's ambient x (base colour x col) with
// the optional gamma 1/2.2, before the quantisation.  col: COLOR_0, or the texture value.
SN_DEV float sn_mesh_shade_channel(float ambient, float base, float col, int gamma) {
#pragma clang fp contract(off)
    float x = ambient * (base * col);
    if (gamma) x = powf(fmaxf(x, 0.0f), 1.0f / 2.2f);
    return x;
}

// One pixel's colour o[0..2]: the background for tri < 0, else triangle `tri` of `tris` shaded at the barycentric weights b0, b1, b2 of
// its corners: interpolated vertex colour x base colour x ambient, optional gamma 1/2.2, unorm8.
SN_DEV void sn_mesh_shade_pixel(const SnMeshShade& s, const int32_t* tris, int tri, float b0, float b1, float b2, uint8_t* o) {
    float rgb[3];
    if (tri < 0) {
        for (int c = 0; c < 3; ++c) rgb[c] = s.background[c];
    } else {
#pragma clang fp contract(off)
        float col[3] = {1.0f, 1.0f, 1.0f};
        if (s.vertex_colors) {
            const int32_t* t = tris + (int64_t)tri * 3;
            const uint8_t* ca = s.vertex_colors + (int64_t)t[0] * 4;
            const uint8_t* cb = s.vertex_colors + (int64_t)t[1] * 4;
            const uint8_t* cc = s.vertex_colors + (int64_t)t[2] * 4;
            for (int c = 0; c < 3; ++c)
                col[c] = b0 * ((float)ca[c] / 255.0f) + b1 * ((float)cb[c] / 255.0f) + b2 * ((float)cc[c] / 255.0f);
        }
        for (int c = 0; c < 3; ++c) rgb[c] = sn_mesh_shade_channel(s.ambient[c], s.base[c], col[c], s.gamma);
    }
    o[0] = sn_unorm8(rgb[0]);
    o[1] = sn_unorm8(rgb[1]);
    o[2] = sn_unorm8(rgb[2]);
}

__global__ __launch_bounds__(SN_MESH_BATCH) void sn_mesh_tile_color_kernel(SnMeshColorParams cp) {
    const SnMeshRasterParams& p = cp.r;
    const SnMeshTileHit h = sn_mesh_tile_sweep<true>(p);
    if (!h.inside) return;
    const int64_t pix = (int64_t)h.py * p.width + h.px;
    if (p.depth) p.depth[pix] = h.z == INFINITY ? 0.0f : h.z;
    float b0 = 1.0f, b1 = 0.0f, b2 = 0.0f;
    if (h.tri >= 0 && cp.s.vertex_colors) {
#pragma clang fp contract(off)
        // the centre is inside (or on an edge of) the winner: e0..e2 share a sign and their sum is not 0 unless the triangle is seen
        // edge-on, where a degenerate weight falls back to the first corner
        const float s = h.e[0] + h.e[1] + h.e[2];
        if (s != 0.0f) {
            b0 = h.e[0] / s;
            b1 = h.e[1] / s;
            b2 = h.e[2] / s;
        }
    }
    sn_mesh_shade_pixel(cp.s, p.tris, h.tri, b0, b1, b2, cp.color + pix * 3);
}

// ------------------------------------------------------------------------------------------
// aabb mode with combine_shape_with_depth (datasetgenerator.py:794-811)
// ------------------------------------------------------------------------------------------
struct SnCombinedMaskParams {
    SnMaskParams m;           // as for K-a / K-b / K-c: m.depth = the NeRF depth
    const float* mesh_depth;  // [H*W] z-depth of the mesh, 0 = not drawn
    const uint8_t* mesh_color;  // [H*W*3], channel 0 read
};

__global__ void sn_mask_condition_combined_kernel(SnCombinedMaskParams cp) {
    const SnMaskParams& p = cp.m;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = (int64_t)p.height * p.width;
    if (i >= n) return;
    if (sn_mask_nothing_visible(p, i)) return;  // (the mesh is not rendered there in the reference)
    p.mask[i] = sn_mask_dilated(p, i) ? 1 : 0;
    if (p.condition) {
#pragma clang fp contract(off)
        float dmin, range;
        sn_mask_depth_norm(p, dmin, range);
        const float dn = (p.depth[i] - dmin) / range;
        const float md = cp.mesh_depth[i];
        const bool cv = (md < p.depth[i]) && (md > 0.0f);  // not inverted by inverse_mask, as in the reference
        const float col = (float)cp.mesh_color[i * 3] / 255.0f;
        // camera_visible_mask * colour + (~camera_visible_mask) * nerf: the multiplies stay (0 * NaN, 0 * inf poison the pixel)
        const float c = (cv ? 1.0f : 0.0f) * col + (cv ? 0.0f : 1.0f) * dn;
        p.condition[i] = sn_mask_one_minus_clamp(c);
    }
}
