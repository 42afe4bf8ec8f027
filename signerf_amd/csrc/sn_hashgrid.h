// sn_hashgrid.h -- the trainable hash grid (include/signerf_hip_hashgrid.h): nerfstudio's torch-path HashEncoding [SURVEY.md A7] on
// caller-owned tables, with its backward pass.  Unlike sn_hash_encode (sn_device.h, the eval path: de-hashed copies, paired tables, a
// handle) these kernels read and write the plain [L*T, F] table a torch Parameter holds.  The formulas are restated in DESIGN.md §4
// "Trainable hash grid"; tests/hashgrid_oracle.py holds them as plain torch ops.
//
// Arithmetic.  Indices and offsets are fp32 exactly as torch computes them: scaled = q * s (ONE IEEE multiply, no contraction), floor
// and ceil to int32, offset = scaled - floor.  The forward blend is the literal fp32 nesting of nerfstudio's (no contraction), so it
// rounds where torch rounds.  The backward pass forms every product in fp64 from the fp32 offsets (1 - o is exact there) and rounds a
// contribution to fp32 ONCE: a grad_table contribution is fl32(wx wy wz g), a grad_q component is fl32 of its whole sum over levels.
//
// Mapping.
//   forward        one thread per (point, level), level fastest: the F features of a thread are contiguous in enc [N, L*F], so a wave
//                  writes one contiguous run; the 8 corner rows of the level are fetched together (one 4F-byte load each).
//   backward_table one thread per (point, level), POINT fastest, the level is blockIdx.y: a wave holds 64 consecutive points -- in
//                  training, consecutive samples of a ray -- at one level.  Reads no table value.  Plain form (variant A): 8 F no-return
//                  fp32 atomic adds per thread.  Merged form (variant B, the levels with scale <= merge_max_scale): lanes that follow
//                  each other with the SAME row are summed in the wave first (a segmented suffix sum over runs of equal rows) and the
//                  first lane of every run issues the add.  Every lane takes part in every shuffle; the step count is a wave vote.
//   backward_input one thread per point, a loop over the levels in order (8 gathers in flight per level), fp64 sums: no shared state,
//                  so grad_q is bit-reproducible.  grad_table is not: float atomics arrive in any order.
//
// Domain.  A point with |q_a * s_l| >= 2^30 for any axis and level, or a non-finite coordinate (the comparison fails for a NaN), is out of
// domain at EVERY level: NaN features, zero index rows, no contribution to grad_table, a NaN grad_q row.  Inside the domain floor and ceil
// fit int32; the row index is masked with T - 1, so no input addresses outside the table.  Element offsets into the table are 32-bit
// (the entry points refuse L * T * F >= 2^31).
//
// Cell policy.  The three kernels take a class G after F that says what a cell IS: the domain, the 8 rows and 3 offsets of a point at a
// level, which corners take 1 - o on which axis, the forward blend and where nerfstudio's corner i sits among the 8.  SnHgTorchGrid (the
// default) is everything above; SnHgTcnnGrid (sn_hashgrid_tcnn.h) is tiny-cuda-nn's grid.  The mapping, the merged atomics and the fp64
// rules are shared.
#pragma once
#include "sn_device.h"

struct SnHashgridParams {
    const float* q;          // [N,3]
    const float* table;      // [L*T,F]
    const float* scal;       // [L]
    const float* grad_enc;   // [N,L*F]
    float* enc;              // [N,L*F]
    int32_t* idx;            // [N,L,8] or null
    float* grad_table;       // [L*T,F], accumulated into
    float* grad_q;           // [N,3]
    int64_t N;
    int32_t L, log2_T;
    float merge_max_scale;   // backward_table<F, true>: levels with scal[l] <= this merge equal rows in the wave
};

#define SN_HG_BLOCK 256
#define SN_HG_LIMIT 1073741824.0f   // 2^30

// corner k of nerfstudio's hashed_0..7 takes the FLOOR coordinate on an axis where its bit is set (0 ccc, 1 cfc, 2 ffc, 3 fcc, 4 ccf,
// 5 cff, 6 fff, 7 fcf; x y z), else the ceil coordinate -- and with it the weight 1 - o, else o
#define SN_HG_XF 0xccu
#define SN_HG_YF 0x66u
#define SN_HG_ZF 0xf0u

template <int F>
struct SnHgRow {
    float v[F];
};

template <int F>
SN_DEV SnHgRow<F> sn_hg_load(const float* p) {
    SnHgRow<F> r;
    if constexpr (F == 1) {
        r.v[0] = p[0];
    } else if constexpr (F == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        r.v[0] = t.x;
        r.v[1] = t.y;
    } else {
#pragma unroll
        for (int i = 0; i < F; i += 4) {
            const float4 t = *reinterpret_cast<const float4*>(p + i);
            r.v[i] = t.x;
            r.v[i + 1] = t.y;
            r.v[i + 2] = t.z;
            r.v[i + 3] = t.w;
        }
    }
    return r;
}

template <int F>
SN_DEV void sn_hg_store(float* p, const SnHgRow<F>& r) {
    if constexpr (F == 1) {
        p[0] = r.v[0];
    } else if constexpr (F == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
    } else {
#pragma unroll
        for (int i = 0; i < F; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(r.v[i], r.v[i + 1], r.v[i + 2], r.v[i + 3]);
    }
}

SN_DEV bool sn_hg_in_domain(const float q[3], const float* scal, int L) {
    bool ok = true;
    for (int l = 0; l < L; ++l) {
        const float s = scal[l];
#pragma unroll
        for (int a = 0; a < 3; ++a) ok = ok && (__builtin_fabsf(q[a] * s) < SN_HG_LIMIT);   // false for a NaN
    }
    return ok;
}

// rows (with the level's offset l * T) and offsets of an in-domain point at level l
SN_DEV void sn_hg_cell(const float q[3], float s, int l, int log2_T, uint32_t row[8], float o[3]) {
#pragma clang fp contract(off)
    uint32_t h[3][2];   // [axis][0 ceil, 1 floor], multiplied by the axis' prime in wrapping uint32: the low bits of torch's int64 product
    const uint32_t prime[3] = {1u, 2654435761u, 805459861u};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = q[a] * s;
        const float fl = __builtin_floorf(x);
        o[a] = x - fl;
        h[a][0] = (uint32_t)(int32_t)__builtin_ceilf(x) * prime[a];
        h[a][1] = (uint32_t)(int32_t)fl * prime[a];
    }
    const uint32_t mask = (1u << log2_T) - 1u, base = (uint32_t)l << log2_T;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        row[k] = ((h[0][(SN_HG_XF >> k) & 1u] ^ h[1][(SN_HG_YF >> k) & 1u] ^ h[2][(SN_HG_ZF >> k) & 1u]) & mask) + base;
}

// nerfstudio's torch-path grid as a cell policy: the functions above, the corner masks, nerfstudio's blend nesting in fp32
struct SnHgTorchGrid {
    static constexpr uint32_t XF = SN_HG_XF, YF = SN_HG_YF, ZF = SN_HG_ZF;
    static constexpr int slot(int i) { return i; }   // where corner i of nerfstudio's order sits in row[] / c[]
    static SN_DEV bool in_domain(const float q[3], const float* scal, int L) { return sn_hg_in_domain(q, scal, L); }
    static SN_DEV void cell(const float q[3], float s, int l, int log2_T, uint32_t row[8], float o[3]) { sn_hg_cell(q, s, l, log2_T, row, o); }
    template <int F>
    static SN_DEV void blend(const SnHgRow<F> c[8], const float o[3], SnHgRow<F>& e) {
#pragma clang fp contract(off)
        const float ox = o[0], oy = o[1], oz = o[2], rx = 1.0f - ox, ry = 1.0f - oy, rz = 1.0f - oz;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float f03 = c[0].v[f] * ox + c[3].v[f] * rx;
            const float f12 = c[1].v[f] * ox + c[2].v[f] * rx;
            const float f56 = c[5].v[f] * ox + c[6].v[f] * rx;
            const float f47 = c[4].v[f] * ox + c[7].v[f] * rx;
            const float f0312 = f03 * oy + f12 * ry;
            const float f4756 = f47 * oy + f56 * ry;
            e.v[f] = f0312 * oz + f4756 * rz;
        }
    }
};

template <int F, class G = SnHgTorchGrid>
__global__ __launch_bounds__(SN_HG_BLOCK) void sn_hashgrid_forward_kernel(SnHashgridParams p) {
    const uint64_t t = (uint64_t)blockIdx.x * SN_HG_BLOCK + threadIdx.x, total = (uint64_t)p.N * (uint32_t)p.L;
    if (t >= total) return;
    int64_t n;
    if (total <= 0xffffffffull) n = (uint32_t)t / (uint32_t)p.L;   // (block-uniform: a 32-bit divide whenever the batch allows it)
    else n = (int64_t)(t / (uint32_t)p.L);
    const int l = (int)(t - (uint64_t)n * (uint32_t)p.L);
    const float q[3] = {p.q[n * 3], p.q[n * 3 + 1], p.q[n * 3 + 2]};
    float* out = p.enc + (int64_t)t * F;
    int32_t* irow = p.idx ? p.idx + (int64_t)t * 8 : nullptr;
    SnHgRow<F> e;
    if (!G::in_domain(q, p.scal, p.L)) {
#pragma unroll
        for (int f = 0; f < F; ++f) e.v[f] = __builtin_nanf("");
        sn_hg_store<F>(out, e);
        if (irow) {
            *reinterpret_cast<int4*>(irow) = make_int4(0, 0, 0, 0);
            *reinterpret_cast<int4*>(irow + 4) = make_int4(0, 0, 0, 0);
        }
        return;
    }
    uint32_t row[8];
    float o[3];
    G::cell(q, p.scal[l], l, p.log2_T, row, o);
    SnHgRow<F> c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = sn_hg_load<F>(p.table + row[k] * (uint32_t)F);
    G::template blend<F>(c, o, e);
    sn_hg_store<F>(out, e);
    if (irow) {
        *reinterpret_cast<int4*>(irow) = make_int4((int)row[0], (int)row[1], (int)row[2], (int)row[3]);
        *reinterpret_cast<int4*>(irow + 4) = make_int4((int)row[4], (int)row[5], (int)row[6], (int)row[7]);
    }
}

// grad_table[row_k] += fl32(wx wy wz g_f): every lane of the block reaches every shuffle (no early return).
template <int F, bool MERGE, class G = SnHgTorchGrid>
__global__ __launch_bounds__(SN_HG_BLOCK) void sn_hashgrid_backward_table_kernel(SnHashgridParams p) {
    const int64_t n = (int64_t)blockIdx.x * SN_HG_BLOCK + threadIdx.x;
    const int l = (int)blockIdx.y;
    float q[3] = {0.0f, 0.0f, 0.0f};
    bool valid = n < p.N;
    if (valid) {
        q[0] = p.q[n * 3];
        q[1] = p.q[n * 3 + 1];
        q[2] = p.q[n * 3 + 2];
        valid = G::in_domain(q, p.scal, p.L);
    }
    const float s = p.scal[l];
    uint32_t row[8] = {};
    float o[3] = {0.0f, 0.0f, 0.0f};
    SnHgRow<F> g{};
    if (valid) {
        G::cell(q, s, l, p.log2_T, row, o);
        g = sn_hg_load<F>(p.grad_enc + (n * p.L + l) * F);
    }
    const double ox = o[0], oy = o[1], oz = o[2];
    const bool merge = MERGE && s <= p.merge_max_scale;   // block-uniform: one level per block
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double w = (((G::XF >> k) & 1u) ? 1.0 - ox : ox) * (((G::YF >> k) & 1u) ? 1.0 - oy : oy) * (((G::ZF >> k) & 1u) ? 1.0 - oz : oz);
        float v[F];
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = (float)(w * (double)g.v[f]);
        bool add = valid;
        if (MERGE && merge) {
            // runs of lanes that follow each other with the same row; an invalid lane is a run of its own kind (key ~0 is no row: the
            // largest row index is L * T - 1 < 2^29) and its values are zeros
            const uint32_t key = valid ? row[k] : 0xffffffffu;
            const uint32_t prev = __shfl_up(key, 1, 64);
            const bool head = lane == 0 || prev != key;
            const unsigned long long heads = __ballot(head);
            const unsigned long long later = lane == 63 ? 0ull : (heads >> (lane + 1));
            const int last = later ? lane + __builtin_ctzll(later) : 63;   // last lane of this lane's run
            for (int d = 1; d < 64; d <<= 1) {
                const bool take = lane + d <= last;
                if (!__any(take)) break;   // wave-uniform: no run is longer than d
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const float t = __shfl_down(v[f], d, 64);
                    if (take) v[f] += t;
                }
            }
            add = valid && head;
        }
        if (add) {
            float* dst = p.grad_table + row[k] * (uint32_t)F;
#pragma unroll
            for (int f = 0; f < F; ++f) atomicAdd(dst + f, v[f]);
        }
    }
}

// grad_q_a = sum_l s_l sum_f g_f d enc_f / d o_a, the literal derivative of the blend
template <int F, class G = SnHgTorchGrid>
__global__ __launch_bounds__(SN_HG_BLOCK) void sn_hashgrid_backward_input_kernel(SnHashgridParams p) {
    const int64_t n = (int64_t)blockIdx.x * SN_HG_BLOCK + threadIdx.x;
    if (n >= p.N) return;
    const float q[3] = {p.q[n * 3], p.q[n * 3 + 1], p.q[n * 3 + 2]};
    float* out = p.grad_q + n * 3;
    if (!G::in_domain(q, p.scal, p.L)) {
        out[0] = out[1] = out[2] = __builtin_nanf("");
        return;
    }
    double gx = 0.0, gy = 0.0, gz = 0.0;
    for (int l = 0; l < p.L; ++l) {
        const float s = p.scal[l];
        uint32_t row[8];
        float o[3];
        G::cell(q, s, l, p.log2_T, row, o);
        SnHgRow<F> c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = sn_hg_load<F>(p.table + row[k] * (uint32_t)F);
        const SnHgRow<F> g = sn_hg_load<F>(p.grad_enc + (n * p.L + l) * F);
        const double ox = o[0], oy = o[1], oz = o[2], rx = 1.0 - ox, ry = 1.0 - oy, rz = 1.0 - oz;
        double dx = 0.0, dy = 0.0, dz = 0.0;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const double f0 = c[G::slot(0)].v[f], f1 = c[G::slot(1)].v[f], f2 = c[G::slot(2)].v[f], f3 = c[G::slot(3)].v[f], f4 = c[G::slot(4)].v[f],
                         f5 = c[G::slot(5)].v[f], f6 = c[G::slot(6)].v[f], f7 = c[G::slot(7)].v[f];
            const double f03 = f0 * ox + f3 * rx, f12 = f1 * ox + f2 * rx, f56 = f5 * ox + f6 * rx, f47 = f4 * ox + f7 * rx;
            const double f0312 = f03 * oy + f12 * ry, f4756 = f47 * oy + f56 * ry;
            const double gf = g.v[f];
            dx += gf * (((f0 - f3) * oy + (f1 - f2) * ry) * oz + ((f4 - f7) * oy + (f5 - f6) * ry) * rz);
            dy += gf * ((f03 - f12) * oz + (f47 - f56) * rz);
            dz += gf * (f0312 - f4756);
        }
        gx += (double)s * dx;
        gy += (double)s * dy;
        gz += (double)s * dz;
    }
    out[0] = (float)gx;
    out[1] = (float)gy;
    out[2] = (float)gz;
}
