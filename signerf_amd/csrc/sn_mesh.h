// sn_mesh.h -- "shape" masking mode: the proxy mesh's depth image and the shape-mode mask + condition
// (signerf/datasetgenerator/datasetgenerator.py:711-754, signerf/renderer/renderer.py:64-196 of the reference).  The reference draws the
// mesh with pyrender (OpenGL / EGL) and reads the depth buffer back per view; here two kernels write the same z-depth image on the
// device:
//   M-a  triangle setup, one thread per triangle: model-view transform, back-face cull, near / far reject, a fixed-size record
//        (three homogeneous edge vectors, the plane, the pixel bbox)
//   M-b  per-tile depth, one 16x16 workgroup per screen tile: sn_mesh_tile_sweep sweeps the triangles' bboxes in batches of 256, compacts
//        the ones that touch the tile into LDS (ballot + prefix: fixed order), then every pixel tests coverage and keeps the nearest t in
//        [znear, zfar].  The colour raster of sn_mesh_color.h (M-e) is the same sweep, instantiated to keep the winning triangle as well.
// No atomics, no data-dependent workspace (its size is a function of the triangle count), bit-identical run to run.  Then the shape
// mode's mask step, from the helpers of sn_mask.h:
//   M-c  visible mask + count / min of the visible mesh depths / max of ALL mesh depths
//   K-b  the dilation prefix counts (sn_mask_prefix_kernel, shared with the aabb mode)
//   M-d  dilation + the shape condition 1 - clamp(vis * obj_norm + !vis * nerf_norm, 0, 1)
#pragma once
#include "sn_device.h"
#include "sn_mask.h"

#define SN_MESH_TILE 16
#define SN_MESH_BATCH 256  // = threads per tile workgroup

// Per-triangle record, 16 words: e0..e2 = B x C, C x A, A x B (coverage of a ray d through the pixel centre: the three d . e have one
// sign), n = (B - A) x (C - A) with nA = n . A (hit distance t = nA / (n . d), which is the z-depth since d.z = -1).
struct SnMeshTri {
    float e[9];
    float n[3];
    float nA;
    float pad[3];
};

struct SnMeshRasterParams {
    const float* vertices;   // [V,3]
    const int32_t* tris;     // [F,3]
    int64_t n_vertices;
    int32_t n_tris;
    float mv[12];            // camera-from-object, row-major 3x4, OpenGL camera (looks down -z)
    float fx, fy, cx, cy;
    int height, width;
    float znear, zfar;
    int cull;
    SnMeshTri* rec;          // [F] workspace
    uint2* bbox;             // [F] workspace: (x0 | y0 << 16, x1 | y1 << 16), inclusive pixel ranges; x0 > x1 = rejected
    float* depth;            // [H,W] out
};

SN_DEV void sn_cross3(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// inclusive range of pixel indices k whose centre k + 0.5 lies in [lo, hi] (coordinates in pixels), padded by one pixel against the
// rounding of the projection, clamped to [0, n - 1].  Empty: a > b.
SN_DEV void sn_mesh_span(float lo, float hi, int n, int& a, int& b) {
    lo = fminf(fmaxf(lo, -2.0f), (float)n + 2.0f);  // also maps -inf / +inf (a vertex on the camera plane) into range
    hi = fminf(fmaxf(hi, -2.0f), (float)n + 2.0f);
    a = max((int)ceilf(lo - 0.5f) - 1, 0);
    b = min((int)floorf(hi - 0.5f) + 1, n - 1);
}

__global__ __launch_bounds__(256) void sn_mesh_setup_kernel(SnMeshRasterParams p) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= p.n_tris) return;
    const uint2 rejected = make_uint2(0xffffu, 0u);
    int idx[3];
    for (int k = 0; k < 3; ++k) {
        idx[k] = p.tris[(int64_t)f * 3 + k];
        if (idx[k] < 0 || (int64_t)idx[k] >= p.n_vertices) {  // never read behind the vertex buffer
            p.bbox[f] = rejected;
            return;
        }
    }
    float v[3][3];
    for (int k = 0; k < 3; ++k) {
        const float* s = p.vertices + (int64_t)idx[k] * 3;
        const float x = s[0], y = s[1], z = s[2];
        for (int r = 0; r < 3; ++r) v[k][r] = fmaf(p.mv[r * 4 + 0], x, fmaf(p.mv[r * 4 + 1], y, fmaf(p.mv[r * 4 + 2], z, p.mv[r * 4 + 3])));
    }
    SnMeshTri t;
    sn_cross3(v[1], v[2], t.e + 0);
    sn_cross3(v[2], v[0], t.e + 3);
    sn_cross3(v[0], v[1], t.e + 6);
    const float ab[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
    const float ac[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
    sn_cross3(ab, ac, t.n);
    t.nA = t.n[0] * v[0][0] + t.n[1] * v[0][1] + t.n[2] * v[0][2];
    t.pad[0] = t.pad[1] = t.pad[2] = 0.0f;
    // camera at the origin: a counter-clockwise (front) face has its normal towards the camera, n . A < 0 (GL_BACK culling)
    const float z0 = -v[0][2], z1 = -v[1][2], z2 = -v[2][2];  // eye depths
    const bool culled = p.cull && !(t.nA < 0.0f);
    const bool outside = (z0 < p.znear && z1 < p.znear && z2 < p.znear) || (z0 > p.zfar && z1 > p.zfar && z2 > p.zfar);
    if (culled || outside || !(t.nA == t.nA)) {
        p.bbox[f] = rejected;
        return;
    }
    int x0 = 0, x1 = p.width - 1, y0 = 0, y1 = p.height - 1;
    if (z0 > 0.0f && z1 > 0.0f && z2 > 0.0f) {
        // wholly in front of the camera plane: the projection of the triangle bounds that of its clipped part
        float ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
        for (int k = 0; k < 3; ++k) {
            const float iz = 1.0f / -v[k][2];
            const float u = fmaf(p.fx, v[k][0] * iz, p.cx);   // column coordinate: pixel j's centre is at j + 0.5
            const float w = fmaf(-p.fy, v[k][1] * iz, p.cy);  // row coordinate (image y points down)
            ulo = fminf(ulo, u);
            uhi = fmaxf(uhi, u);
            vlo = fminf(vlo, w);
            vhi = fmaxf(vhi, w);
        }
        sn_mesh_span(ulo, uhi, p.width, x0, x1);
        sn_mesh_span(vlo, vhi, p.height, y0, y1);
        if (x0 > x1 || y0 > y1) {
            p.bbox[f] = rejected;
            return;
        }
    }  // else it crosses the camera plane: conservative whole-image bbox, the homogeneous edge test does the rest
    p.rec[f] = t;
    p.bbox[f] = make_uint2((uint32_t)x0 | ((uint32_t)y0 << 16), (uint32_t)x1 | ((uint32_t)y1 << 16));
}

// What one thread of a tile workgroup knows after the sweep.  tri and e are kept by the kColor instantiation only.
struct SnMeshTileHit {
    int px, py;   // this thread's pixel
    bool inside;  // ... is inside the image (the tiles of the last column / row hang over)
    float z;      // nearest depth in [znear, zfar], INFINITY: nothing covers the pixel centre
    int tri;      // the triangle of z, -1: none
    float e[3];   // its three edge values at this pixel
};

// The per-tile loop of M-b and M-e, called by all SN_MESH_BATCH threads of the tile (blockIdx.x, blockIdx.y).  Ties in z go to the
// triangle met first (strict z < best): batches and their LDS compaction are in triangle order, so the lowest index wins, as GL_LESS
// keeps the first drawn.  z > 0 here, so for the depth alone the strict update keeps what fminf(best, z) would.
template <bool kColor>
SN_DEV SnMeshTileHit sn_mesh_tile_sweep(const SnMeshRasterParams& p) {
    __shared__ SnMeshTri s_rec[SN_MESH_BATCH];
    __shared__ int s_idx[SN_MESH_BATCH];
    __shared__ int s_wave[SN_MESH_BATCH / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * SN_MESH_TILE, ty0 = blockIdx.y * SN_MESH_TILE;
    const int tx1 = min(tx0 + SN_MESH_TILE, p.width) - 1, ty1 = min(ty0 + SN_MESH_TILE, p.height) - 1;
    SnMeshTileHit h;
    h.px = tx0 + (tid % SN_MESH_TILE);
    h.py = ty0 + (tid / SN_MESH_TILE);
    h.inside = h.px <= tx1 && h.py <= ty1;
    h.z = INFINITY;
    h.tri = -1;
    h.e[0] = h.e[1] = h.e[2] = 0.0f;
    float dx, dy;
    {
#pragma clang fp contract(off)
        dx = ((float)h.px + 0.5f - p.cx) / p.fx;
        dy = -(((float)h.py + 0.5f - p.cy) / p.fy);
    }
    const float dz = -1.0f;
    for (int base = 0; base < p.n_tris; base += SN_MESH_BATCH) {
        // 1. which triangles of this batch touch the tile: fixed-order compaction (ballot + wave prefix)
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
        // 2. stage the records of those triangles
        if (tid < total) s_rec[tid] = p.rec[s_idx[tid]];
        __syncthreads();
        // 3. every pixel against every staged triangle, in index order (the loop bound is uniform over the workgroup)
        for (int k = 0; k < total; ++k) {
            const SnMeshTri& t = s_rec[k];
            const float e0 = fmaf(t.e[0], dx, fmaf(t.e[1], dy, t.e[2] * dz));
            const float e1 = fmaf(t.e[3], dx, fmaf(t.e[4], dy, t.e[5] * dz));
            const float e2 = fmaf(t.e[6], dx, fmaf(t.e[7], dy, t.e[8] * dz));
            const bool in = (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) || (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
            if (in) {
                const float nd = fmaf(t.n[0], dx, fmaf(t.n[1], dy, t.n[2] * dz));
                const float z = t.nA / nd;  // NaN / inf for a ray in the plane: fails the comparisons below
                if (z >= p.znear && z <= p.zfar && z < h.z) {
                    h.z = z;
                    if constexpr (kColor) {
                        h.tri = s_idx[k];
                        h.e[0] = e0;
                        h.e[1] = e1;
                        h.e[2] = e2;
                    }
                }
            }
        }
        __syncthreads();  // s_wave / s_idx / s_rec are rewritten by the next batch
    }
    return h;
}

__global__ __launch_bounds__(SN_MESH_BATCH) void sn_mesh_tile_kernel(SnMeshRasterParams p) {
    const SnMeshTileHit h = sn_mesh_tile_sweep<false>(p);
    if (h.inside) p.depth[(int64_t)h.py * p.width + h.px] = h.z == INFINITY ? 0.0f : h.z;
}

// ------------------------------------------------------------------------------------------
// shape-mode mask + condition (datasetgenerator.py:716-754)
// ------------------------------------------------------------------------------------------
struct SnShapeMaskParams {
    SnMaskParams m;           // m.depth = the NeRF depth; m.stats[0] count, [1] ordered min of the visible mesh depths, [2] ordered max of all
    const float* mesh_depth;  // [H*W] z-depth of the mesh, 0 = not drawn
};

__global__ __launch_bounds__(256) void sn_shape_visible_kernel(SnShapeMaskParams sp) {
    const SnMaskParams& p = sp.m;
    const int64_t n = (int64_t)p.height * p.width;
    uint32_t cnt = 0u, lo = 0xffffffffu, hi = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float md = sp.mesh_depth[i], nd = p.depth[i];
        bool vis = (md < nd) && (md > 0.0f);
        if (p.inverse_mask) vis = !vis;
        p.vis[i] = vis ? 1 : 0;
        cnt += vis ? 1u : 0u;
        const uint32_t om = sn_float_ordered(md);
        if (vis && (md * 1.0f > 0.0f)) lo = min(lo, om);  // depth[visible_mask * depth > 0]
        hi = max(hi, om);                                 // torch.max(depth): every pixel
    }
    sn_mask_block_reduce(cnt, lo, hi);
    if (threadIdx.x == 0) {
        if (cnt) atomicAdd(&p.stats[0], cnt);
        if (lo != 0xffffffffu) atomicMin(&p.stats[1], lo);
        atomicMax(&p.stats[2], hi);
    }
}

__global__ void sn_shape_condition_kernel(SnShapeMaskParams sp) {
#pragma clang fp contract(off)
    const SnMaskParams& p = sp.m;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = (int64_t)p.height * p.width;
    if (i >= n) return;
    if (sn_mask_nothing_visible(p, i)) return;
    const bool v = p.vis[i] != 0;
    p.mask[i] = sn_mask_dilated(p, i) ? 1 : 0;
    if (!p.condition) return;
    if (!p.has_manual_depth && p.stats[1] == 0xffffffffu) {
        // something is visible but no visible pixel has a mesh depth > 0 (reachable with inverse_mask): the reference's torch.min of an
        // empty selection raises.  Defined here as an all-zero condition (the mask stays as computed).
        p.condition[i] = 0.0f;
        return;
    }
    float dmin, range;
    sn_mask_depth_norm(p, dmin, range);
    const float on = (sp.mesh_depth[i] - dmin) / range;
    const float nn = (p.depth[i] - dmin) / range;
    // visible_mask * obj + (~visible_mask) * nerf: the multiplies stay (0 * NaN, 0 * inf = NaN poisons the pixel as in the reference)
    const float c = (v ? 1.0f : 0.0f) * on + (v ? 0.0f : 1.0f) * nn;
    p.condition[i] = sn_mask_one_minus_clamp(c);
}
