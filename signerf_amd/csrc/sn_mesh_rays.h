// sn_mesh_rays.h -- the proxy mesh drawn by casting the camera's own rays (RendererConfig.lens = "camera"): the depth and colour images
// of sn_mesh.h / sn_mesh_color.h for a camera that is not an ideal pinhole (OPENCV distortion, FISHEYE, EQUIRECTANGULAR), from the
// per-pixel world-space rays of sn_generate_rays_camera.  One kernel:
//   M-r  lane = one ray, wave = an 8x8 pixel tile, workgroup = 2x2 tiles (the mapping of the render kernels, sn_main.h): the lanes of a
//        wave walk the same part of the tree.  Closest hit through a two-wide BVH over the posed mesh, built on the host once per mesh
//        (signerf_amd/renderer.py build_accel) and passed as an opaque blob; the traversal stack lives in LDS ([level][thread], one bank
//        per lane), so no array is indexed dynamically in registers and nothing spills.
// What is written is the rasteriser's quantity: the z-depth along the camera axis, z = t * f with f = direction . forward, of the nearest
// DRAWN hit -- f > 0, znear < z < zfar and, with culling, a front-facing (counter-clockwise) triangle; hits that are not drawn do not
// occlude, as the rasteriser clips and culls before its depth test.  A ray that points backwards (f <= 0: the rear hemisphere of an
// EQUIRECTANGULAR camera, a FISHEYE beyond 180 degrees) draws nothing, as a frustum draws nothing behind its camera.  Of two hits at the
// same distance the triangle with the lower index wins.  No atomics: bit-identical run to run.
//
// The blob (version 1; all offsets from its 16-byte-aligned base, sizes in sn_mesh_accel_bytes of sn_api.hip):
//   [0, 64)                     SnMeshAccelHeader
//   [64, 64 + 64 * max(F, 1))   SnMeshAccelNode[n_nodes], node 0 = the root (the rest of the range is padding)
//   then                        SnMeshAccelTri[F], in leaf order
// Every index the kernel takes from the blob is checked against these sizes and the walk is bounded by the node count, so a damaged
// blob gives a wrong image, never an access outside it or an endless loop.
#pragma once
#include "sn_device.h"
#include "sn_mesh_color.h"

#define SN_RAYS_BLOCK 256
#define SN_RAYS_STACK 32          // a median-split tree over F <= 2^26 triangles is at most 26 levels deep
#define SN_RAYS_LEAF_MAX 4
#define SN_RAYS_MAGIC 0x31524d53u  // "SMR1"
#define SN_RAYS_BLOB_VERSION 1u

struct SnMeshAccelHeader {
    uint32_t magic, version, n_tris, n_nodes;
    uint32_t pad[12];
};

// An inner node holds the boxes of its two children.  A child >= 0 is an inner node; a child < 0 is a leaf -(1 + first * 8 + count) of
// count <= SN_RAYS_LEAF_MAX triangles from `first` (count 0 with an inverted box: no child).
struct SnMeshAccelNode {
    float lmin[3], lmax[3], rmin[3], rmax[3];
    int32_t left, right, pad[2];
};

struct SnMeshAccelTri {
    float a[3], b[3], c[3];  // the posed (world-space) corners
    int32_t index;           // the triangle's index in the caller's triangle array
    int32_t pad[2];
};

static_assert(sizeof(SnMeshAccelHeader) == 64 && sizeof(SnMeshAccelNode) == 64 && sizeof(SnMeshAccelTri) == 48, "blob layout");

struct SnMeshRaysParams {
    const float* origins;     // [H*W,3]
    const float* directions;  // [H*W,3]
    int height, width;
    float fwd[3];             // the camera's viewing axis (unit, world space)
    float znear, zfar;
    int cull;
    const uint8_t* accel;
    int32_t n_tris;
    const int32_t* tris;      // [F,3], read for the vertex colours only
    int64_t n_vertices;
    SnMeshShade s;
    float* depth;             // [H*W] out
    uint8_t* color;           // [H*W,3] out, or NULL
};

struct SnRayHit {
    float t;      // distance of the nearest drawn hit in units of |direction|, INFINITY: none
    float u, v;   // its barycentric weights of corners b and c
    int tri;      // its index in the caller's triangle array, -1: none
};

// distance at which the ray enters the box, or INFINITY when it misses it or enters beyond `limit`.  The three products carry a relative
// error of a few ulp each; the exit distance is widened by 1 + 2^-21 so that a box is never missed for it (Ize, "Robust BVH ray
// traversal", 2013).
SN_DEV float sn_ray_box(const float* lo, const float* hi, const float* o, const float* inv, float limit) {
    float tn = 0.0f, tf = limit;
    for (int k = 0; k < 3; ++k) {
        const float t0 = (lo[k] - o[k]) * inv[k], t1 = (hi[k] - o[k]) * inv[k];
        tn = fmaxf(tn, fminf(t0, t1));  // fminf / fmaxf drop a NaN (0 * inf)
        tf = fminf(tf, fmaxf(t0, t1) * 1.0000005f);
    }
    return tn <= tf ? tn : INFINITY;
}

// Moeller-Trumbore against the triangles of the leaf `child` (< 0, SnMeshAccelNode)
SN_DEV void sn_ray_leaf(const SnMeshAccelTri* tris, int child, const float* o, const float* d, float f, const SnMeshRaysParams& p, SnRayHit& h) {
    const int ref = -(child + 1), first = ref >> 3, count = ref & 7;
    if (count > SN_RAYS_LEAF_MAX || first + count > p.n_tris) return;
    for (int k = 0; k < count; ++k) {
        const f32x4* q = (const f32x4*)(tris + first + k);
        const f32x4 q0 = q[0], q1 = q[1], q2 = q[2];
        const float a[3] = {q0.x, q0.y, q0.z};
        const float e1[3] = {q0.w - a[0], q1.x - a[1], q1.y - a[2]};
        const float e2[3] = {q1.z - a[0], q1.w - a[1], q2.x - a[2]};
        const int index = __float_as_int(q2.y);
        float pv[3], qv[3];
        sn_cross3(d, e2, pv);
        const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];  // = -(direction . normal): > 0 for a front face
        if (p.cull ? !(det > 0.0f) : det == 0.0f) continue;
        const float inv = 1.0f / det;
        const float tv[3] = {o[0] - a[0], o[1] - a[1], o[2] - a[2]};
        const float u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv;
        sn_cross3(tv, e1, qv);
        const float v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) * inv;
        const float t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv;
        const float z = t * f;
        // (a NaN fails every comparison)
        if (u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t > 0.0f && z > p.znear && z < p.zfar && (t < h.t || (t == h.t && index < h.tri))) {
            h.t = t;
            h.u = u;
            h.v = v;
            h.tri = index;
        }
    }
}

// The walk of M-r, called by all SN_RAYS_BLOCK threads of the workgroup (blockIdx.x, blockIdx.y): this thread's ray (false: its pixel
// is outside the image), f = direction . forward, and the nearest drawn hit.  The kernels below and the one of sn_mesh_material.h differ
// in what they write for it.
SN_DEV bool sn_mesh_rays_walk(const SnMeshRaysParams& p, int64_t& ray, float& f, SnRayHit& h) {
    __shared__ int s_stack[SN_RAYS_STACK][SN_RAYS_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int px = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), py = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (px >= p.width || py >= p.height) return false;  // (no barrier below)
    ray = (int64_t)py * p.width + px;
    const float o[3] = {p.origins[ray * 3 + 0], p.origins[ray * 3 + 1], p.origins[ray * 3 + 2]};
    const float d[3] = {p.directions[ray * 3 + 0], p.directions[ray * 3 + 1], p.directions[ray * 3 + 2]};
    f = d[0] * p.fwd[0] + d[1] * p.fwd[1] + d[2] * p.fwd[2];
    h.t = INFINITY;
    h.u = h.v = 0.0f;
    h.tri = -1;
    const SnMeshAccelHeader* hd = (const SnMeshAccelHeader*)p.accel;
    const uint32_t n_nodes = hd->n_nodes;
    const uint32_t cap = (uint32_t)max(p.n_tris, 1);
    const bool blob_ok = hd->magic == SN_RAYS_MAGIC && hd->version == SN_RAYS_BLOB_VERSION && hd->n_tris == (uint32_t)p.n_tris && n_nodes >= 1u &&
                         n_nodes <= cap;
    if (blob_ok && f > 0.0f) {
        const SnMeshAccelNode* nodes = (const SnMeshAccelNode*)(p.accel + sizeof(SnMeshAccelHeader));
        const SnMeshAccelTri* tris = (const SnMeshAccelTri*)(p.accel + sizeof(SnMeshAccelHeader) + (size_t)cap * sizeof(SnMeshAccelNode));
        float inv[3];
        for (int k = 0; k < 3; ++k) inv[k] = fabsf(d[k]) >= 1e-20f ? 1.0f / d[k] : copysignf(1e20f, d[k]);
        int sp = 0;
        uint32_t node = 0u;
        // every inner node of a tree is entered once: 2 * n_nodes steps end the walk over a blob that is not one
        for (uint32_t step = 0u; step < 2u * n_nodes && node < n_nodes; ++step) {
            const f32x4* q = (const f32x4*)(nodes + node);
            const f32x4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            const float lmin[3] = {q0.x, q0.y, q0.z}, lmax[3] = {q0.w, q1.x, q1.y};
            const float rmin[3] = {q1.z, q1.w, q2.x}, rmax[3] = {q2.y, q2.z, q2.w};
            int cl = __float_as_int(q3.x), cr = __float_as_int(q3.y);
            float tl = sn_ray_box(lmin, lmax, o, inv, h.t);
            if (cl < 0) {  // a leaf: nothing to descend into
                if (tl != INFINITY) sn_ray_leaf(tris, cl, o, d, f, p, h);
                tl = INFINITY;
            }
            float tr = sn_ray_box(rmin, rmax, o, inv, h.t);
            if (cr < 0) {
                if (tr != INFINITY) sn_ray_leaf(tris, cr, o, d, f, p, h);
                tr = INFINITY;
            }
            if (tl != INFINITY && tr != INFINITY) {  // the nearer child first, the other one for later
                const bool right_first = tr < tl;
                if (sp < SN_RAYS_STACK) s_stack[sp++][tid] = right_first ? cl : cr;
                node = (uint32_t)(right_first ? cr : cl);
            } else if (tl != INFINITY) {
                node = (uint32_t)cl;
            } else if (tr != INFINITY) {
                node = (uint32_t)cr;
            } else if (sp > 0) {
                node = (uint32_t)s_stack[--sp][tid];
            } else {
                break;
            }
        }
    }
    return true;
}

template <bool kColor>
__global__ __launch_bounds__(SN_RAYS_BLOCK) void sn_mesh_rays_kernel(SnMeshRaysParams p) {
    int64_t ray;
    float f;
    SnRayHit h;
    if (!sn_mesh_rays_walk(p, ray, f, h)) return;
    const bool drawn = h.tri >= 0;
    p.depth[ray] = drawn ? h.t * f : 0.0f;
    if constexpr (kColor) {
        int tri = drawn && h.tri < p.n_tris ? h.tri : -1;
        if (tri >= 0 && p.s.vertex_colors) {
            for (int k = 0; k < 3; ++k) {  // never read behind the colour buffer
                const int32_t i = p.tris[(int64_t)tri * 3 + k];
                if (i < 0 || (int64_t)i >= p.n_vertices) tri = -1;
            }
        }
        sn_mesh_shade_pixel(p.s, p.tris, tri, 1.0f - h.u - h.v, h.u, h.v, p.color + ray * 3);
    }
}
