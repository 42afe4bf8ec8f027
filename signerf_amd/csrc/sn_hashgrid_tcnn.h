// sn_hashgrid_tcnn.h -- tiny-cuda-nn's multiresolution grid as a cell policy of the trainable hash-grid kernels (sn_hashgrid.h), for
// signerf_amd/include/signerf_hip_hashgrid_tcnn.h.  The table is the uniform [L*T, F] one signerf_amd/tcnn_import.py produces: a level the library
// indexes densely occupies the first n_l rows of its slot of T.  The semantics are oracle/tcnn_layout.py's (grid_meta, grid_rows,
// grid_encode), restated in DESIGN.md §4 "Trainable tcnn grid"; tests/tcnn_hashgrid_oracle.py holds them as plain torch ops.
//
// Per point and level: x = fmaf(s, q, 0.5) (one rounding), c = floor(x), w = x - c.  Corner k = 0..7 adds 1 on axis a where bit a of k is
// set and weighs w_a there, 1 - w_a elsewhere.  r = ceil(s) + 1, n = min(next_multiple(r^3, 8), T); the level is dense iff r^3 <= n and
// then reads row (x + y r + z r^2) in wrapping uint32, % n (a true modulo); else the xor hash & (T - 1).  Both + l T.
//
// Arithmetic.  The forward blend is grid_encode's order in fp32 without contraction -- weight = ((1 wx) wy) wz, acc += weight row, corner
// 0 first -- so it rounds where the restatement rounds.  The backward pass is sn_hashgrid.h's: fp64 products of the fp32 weights, one
// rounding per contribution; grad_q by the same fp64 derivative of the trilinear blend, the corners taken in nerfstudio's order (slot).
//
// Domain.  In domain iff every x, on every axis and level, is finite and in [0, 2^30): floor fits uint32 with room for the + 1.  A negative
// x is undefined in the library and is refused, not guessed.  No input addresses outside its level's slot: a dense row is < n <= T, a
// hashed one is masked, whatever the scalings hold (sn_tcnn_level clamps what it derives from them).
#pragma once
#include "sn_hashgrid.h"

#ifndef SN_HOST_DEV
#define SN_HOST_DEV __host__ __device__ __forceinline__
#endif

#define SN_TCNN_MAX_RES 256u   // a dense level has r^3 <= T <= 2^24

struct SnTcnnLevel {
    uint32_t res, rows;   // r, n
    bool dense;
};

// THE definition of a level's geometry from (s, log2_T): the kernels and the host query sn_hashgrid_tcnn_levels both call it.  ceil(s) is
// clamped to [0, 2^20] (a NaN counts as 0) so that r^3 fits 64 bits and n >= 8 whatever s holds; oracle.tcnn_layout.grid_meta's
// min(r^3, (2^32 - 1) / 2) is the same cap the library applies before it rounds up to 8.
SN_HOST_DEV SnTcnnLevel sn_tcnn_level(float s, int log2_T) {
    float c = __builtin_ceilf(s);
    c = c > 0.0f ? (c < 1048576.0f ? c : 1048576.0f) : 0.0f;
    const uint32_t r = (uint32_t)c + 1u, T = 1u << log2_T;
    const uint64_t r3 = (uint64_t)r * r * r, capped = r3 < 0x7fffffffull ? r3 : 0x7fffffffull;
    const uint64_t n8 = (capped + 7ull) & ~7ull;
    SnTcnnLevel v;
    v.res = r;
    v.rows = (uint32_t)(n8 < T ? n8 : T);
    v.dense = r3 <= v.rows;
    return v;
}

struct SnHgTcnnGrid {
    // corner k takes 1 - w on an axis where its bit is CLEAR
    static constexpr uint32_t XF = 0x55u, YF = 0x33u, ZF = 0x0fu;
    // nerfstudio's corner i (0 ccc, 1 cfc, 2 ffc, 3 fcc, 4 ccf, 5 cff, 6 fff, 7 fcf; c = + 1) is corner slot(i) here
    static constexpr int slot(int i) { return (int)((0x20136457u >> (4 * i)) & 7u); }

    static SN_DEV bool in_domain(const float q[3], const float* scal, int L) {
        bool ok = true;
        for (int l = 0; l < L; ++l) {
            const float s = scal[l];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float x = __builtin_fmaf(s, q[a], 0.5f);
                ok = ok && x >= 0.0f && x < SN_HG_LIMIT;   // false for a NaN
            }
        }
        return ok;
    }

    // rows (with the level's offset l * T) and weights w of an in-domain point at level l
    static SN_DEV void cell(const float q[3], float s, int l, int log2_T, uint32_t row[8], float o[3]) {
        uint32_t c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = __builtin_fmaf(s, q[a], 0.5f);
            const float fl = __builtin_floorf(x);
            o[a] = x - fl;
            c[a] = (uint32_t)fl;   // 0 <= fl < 2^30
        }
        const SnTcnnLevel lv = sn_tcnn_level(s, log2_T);
        const uint32_t base = (uint32_t)l << log2_T;
        if (lv.dense) {
            // (i0 + d_k) mod 2^32, % n.  d_k <= 1 + r + r^2 < n, so off one modulo for i0 the corners cost a compare each -- unless the
            // 32-bit sum wraps (i0 within r^2 + r + 1 of 2^32: coordinates near 2^30), where the corner takes its own modulo
            const uint32_t r = lv.res, r2 = r * r, n = lv.rows;
            const uint32_t i0 = c[0] + c[1] * r + c[2] * r2;
            const uint32_t m = i0 % n;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t d = (uint32_t)(k & 1) + ((k >> 1) & 1) * r + ((k >> 2) & 1) * r2;
                const uint32_t t = i0 + d;
                uint32_t v = m + d;
                v = v >= n ? v - n : v;
                if (__builtin_expect(t < i0, 0)) v = t % n;
                row[k] = v + base;
            }
        } else {
            const uint32_t prime[3] = {1u, 2654435761u, 805459861u};
            uint32_t h[3][2];   // [axis][0: c, 1: c + 1] times the axis' prime, wrapping
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                h[a][0] = c[a] * prime[a];
                h[a][1] = h[a][0] + prime[a];
            }
            const uint32_t mask = (1u << log2_T) - 1u;
#pragma unroll
            for (int k = 0; k < 8; ++k) row[k] = ((h[0][k & 1] ^ h[1][(k >> 1) & 1] ^ h[2][(k >> 2) & 1]) & mask) + base;
        }
    }

    template <int F>
    static SN_DEV void blend(const SnHgRow<F> c[8], const float o[3], SnHgRow<F>& e) {
#pragma clang fp contract(off)
        const float r[3] = {1.0f - o[0], 1.0f - o[1], 1.0f - o[2]};
#pragma unroll
        for (int f = 0; f < F; ++f) e.v[f] = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float w = (((k & 1) ? o[0] : r[0]) * ((k & 2) ? o[1] : r[1])) * ((k & 4) ? o[2] : r[2]);
#pragma unroll
            for (int f = 0; f < F; ++f) e.v[f] = e.v[f] + w * c[k].v[f];
        }
    }
};
