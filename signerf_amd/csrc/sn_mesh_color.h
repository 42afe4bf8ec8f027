// sn_mesh_color.h -- the proxy mesh's COLOUR image and the aabb mode's combine_shape_with_depth condition
// (/root/reference/signerf/datasetgenerator/datasetgenerator.py:794-811, signerf/renderer/renderer.py:64-196).  The reference renders the
// mesh with pyrender in a scene lit by an ambient light of 1 only and pastes channel 0 of the colour image into the ControlNet condition
// wherever the mesh is in front of the NeRF.  Here:
//   M-a  sn_mesh_setup_kernel of sn_mesh.h, unchanged
//   M-e  per-tile colour + depth: M-b's sweep, keeping besides the nearest depth the winning triangle (strict z < best: batches and their
//        LDS compaction are in triangle order, so the lowest index wins a tie, as GL_LESS keeps the first drawn) and its three edge values
//        e0..e2 -- normalised by their sum, the ray's perspective-correct barycentrics.  Per-pixel epilogue: interpolated vertex colour
//        x base colour x ambient, optional gamma 1/2.2, unorm8; background where nothing covers the centre.
//   K-a, K-b of sn_mask.h, unchanged, then
//   K-d  the mask exactly as K-c, and the condition 1 - clamp(cv * colour[0] / 255 + !cv * nerf_norm, 0, 1),
//        cv = (mesh_depth < depth) & (mesh_depth > 0)
// No atomics in M-e (bit-identical run to run); the depth M-e writes is bit-identical to M-b's.
#pragma once
#include "sn_device.h"
#include "sn_mask.h"
#include "sn_mesh.h"

struct SnMeshColorParams {
    SnMeshRasterParams r;         // r.depth may be NULL here
    const uint8_t* vertex_colors; // [V,4] RGBA8, or NULL (COLOR_0 = 1)
    float base[3];                // material baseColorFactor.rgb
    float ambient[3];
    float background[3];          // in [0, 1], written without gamma
    int gamma;                    // != 0: pow(x, 1 / 2.2) before the quantisation
    uint8_t* color;               // [H,W,3] out
};

SN_DEV uint8_t sn_unorm8(float x) {
#pragma clang fp contract(off)
    x = fminf(fmaxf(x, 0.0f), 1.0f);  // (also maps a NaN to 0)
    return (uint8_t)(int)(x * 255.0f + 0.5f);
}

__global__ __launch_bounds__(SN_MESH_BATCH) void sn_mesh_tile_color_kernel(SnMeshColorParams cp) {
    const SnMeshRasterParams& p = cp.r;
    __shared__ SnMeshTri s_rec[SN_MESH_BATCH];
    __shared__ int s_idx[SN_MESH_BATCH];
    __shared__ int s_wave[SN_MESH_BATCH / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * SN_MESH_TILE, ty0 = blockIdx.y * SN_MESH_TILE;
    const int tx1 = min(tx0 + SN_MESH_TILE, p.width) - 1, ty1 = min(ty0 + SN_MESH_TILE, p.height) - 1;
    const int px = tx0 + (tid % SN_MESH_TILE), py = ty0 + (tid / SN_MESH_TILE);
    float dx, dy;
    {
#pragma clang fp contract(off)
        dx = ((float)px + 0.5f - p.cx) / p.fx;
        dy = -(((float)py + 0.5f - p.cy) / p.fy);
    }
    const float dz = -1.0f;
    float best = INFINITY;
    int win = -1;                   // triangle index of `best`
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;  // its edge values at this pixel
    for (int base = 0; base < p.n_tris; base += SN_MESH_BATCH) {
        // 1.-2. as sn_mesh_tile_kernel: fixed-order compaction of the batch's triangles that touch the tile, records staged in LDS
        const int f = base + tid;
        bool hit = false;
        if (f < p.n_tris) {
            const uint2 b = p.bbox[f];
            const int bx0 = (int)(b.x & 0xffffu), by0 = (int)(b.x >> 16), bx1 = (int)(b.y & 0xffffu), by1 = (int)(b.y >> 16);
            hit = !(bx0 > tx1 || bx1 < tx0 || by0 > ty1 || by1 < ty0);
        }
        const uint64_t bal = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < SN_MESH_BATCH / 64; ++w) {
            off += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (hit) s_idx[off + __popcll(bal & ((1ull << lane) - 1ull))] = f;
        __syncthreads();
        if (tid < total) s_rec[tid] = p.rec[s_idx[tid]];
        __syncthreads();
        // 3. every pixel against every staged triangle, in index order; the same arithmetic as sn_mesh_tile_kernel, so the same depth
        for (int k = 0; k < total; ++k) {
            const SnMeshTri& t = s_rec[k];
            const float e0 = fmaf(t.e[0], dx, fmaf(t.e[1], dy, t.e[2] * dz));
            const float e1 = fmaf(t.e[3], dx, fmaf(t.e[4], dy, t.e[5] * dz));
            const float e2 = fmaf(t.e[6], dx, fmaf(t.e[7], dy, t.e[8] * dz));
            const bool in = (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) || (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
            if (in) {
                const float nd = fmaf(t.n[0], dx, fmaf(t.n[1], dy, t.n[2] * dz));
                const float z = t.nA / nd;
                // z > 0 here, so `z < best` keeps what fminf(best, z) keeps; strict: the first (lowest-index) triangle wins a tie
                if (z >= p.znear && z <= p.zfar && z < best) {
                    best = z;
                    win = s_idx[k];
                    w0 = e0;
                    w1 = e1;
                    w2 = e2;
                }
            }
        }
        __syncthreads();  // s_wave / s_idx / s_rec are rewritten by the next batch
    }
    if (px > tx1 || py > ty1) return;
    const int64_t pix = (int64_t)py * p.width + px;
    if (p.depth) p.depth[pix] = best == INFINITY ? 0.0f : best;
    float rgb[3];
    if (win < 0) {
        for (int c = 0; c < 3; ++c) rgb[c] = cp.background[c];
    } else {
#pragma clang fp contract(off)
        float col[3] = {1.0f, 1.0f, 1.0f};
        if (cp.vertex_colors) {
            // the centre is inside (or on an edge of) the winner: e0..e2 share a sign and their sum is not 0 unless the triangle is seen
            // edge-on, where a degenerate weight falls back to the first corner
            const float s = w0 + w1 + w2;
            const float b0 = s != 0.0f ? w0 / s : 1.0f, b1 = s != 0.0f ? w1 / s : 0.0f, b2 = s != 0.0f ? w2 / s : 0.0f;
            const int32_t* tri = p.tris + (int64_t)win * 3;
            const uint8_t* ca = cp.vertex_colors + (int64_t)tri[0] * 4;
            const uint8_t* cb = cp.vertex_colors + (int64_t)tri[1] * 4;
            const uint8_t* cc = cp.vertex_colors + (int64_t)tri[2] * 4;
            for (int c = 0; c < 3; ++c)
                col[c] = b0 * ((float)ca[c] / 255.0f) + b1 * ((float)cb[c] / 255.0f) + b2 * ((float)cc[c] / 255.0f);
        }
        for (int c = 0; c < 3; ++c) {
            float x = cp.ambient[c] * (cp.base[c] * col[c]);
            if (cp.gamma) x = powf(fmaxf(x, 0.0f), 1.0f / 2.2f);
            rgb[c] = x;
        }
    }
    uint8_t* o = cp.color + pix * 3;
    o[0] = sn_unorm8(rgb[0]);
    o[1] = sn_unorm8(rgb[1]);
    o[2] = sn_unorm8(rgb[2]);
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
    const uint32_t count = p.stats[0];
    if (count == 0) {  // is_visible == False: zero mask, zero condition (:812-818); the mesh is not rendered there in the reference
        p.mask[i] = 0;
        if (p.condition) p.condition[i] = 0.0f;
        return;
    }
    const int y = (int)(i / p.width), x = (int)(i % p.width);
    bool m = p.vis[i] != 0;
    if (p.dilate) {  // as sn_mask_condition_kernel
        m = false;
        for (int r = 0; r < p.el.kh && !m; ++r) {
            const int yy = y + r - p.el.ay;
            if (yy < 0 || yy >= p.height) continue;
            const int a = max(x + p.el.j1[r] - p.el.ax, 0), b = min(x + p.el.j2[r] - p.el.ax, p.width);
            if (a >= b) continue;
            const int32_t* pr = p.prefix + (int64_t)yy * (p.width + 1);
            m = pr[b] - pr[a] > 0;
        }
    }
    p.mask[i] = m ? 1 : 0;
    if (p.condition) {
#pragma clang fp contract(off)
        float dmin, range;
        if (p.has_manual_depth) {
            dmin = p.manual_min;
            range = p.manual_range;
        } else {  // as sn_mask_condition_kernel
            dmin = sn_ordered_float(p.stats[1]) - p.depth_radius;
            const float dmax = sn_ordered_float(p.stats[2]) + p.depth_radius;
            range = dmax - dmin;
        }
        const float dn = (p.depth[i] - dmin) / range;
        const float md = cp.mesh_depth[i];
        const bool cv = (md < p.depth[i]) && (md > 0.0f);  // not inverted by inverse_mask, as in the reference
        const float col = (float)cp.mesh_color[i * 3] / 255.0f;
        // camera_visible_mask * colour + (~camera_visible_mask) * nerf: the multiplies stay (0 * NaN, 0 * inf poison the pixel)
        const float c = (cv ? 1.0f : 0.0f) * col + (cv ? 0.0f : 1.0f) * dn;
        p.condition[i] = 1.0f - (c != c ? c : fminf(fmaxf(c, 0.0f), 1.0f));
    }
}
