// sn_hashgrid_ordered.h -- the ordered form of the hash grids' table gradient (signerf_amd/include/signerf_hip_hashgrid_ordered.h): store
// every contribution once, sort (row, contribution id) per level, sum every row's list in fp64 in ascending id order.  No float atomics,
// so two calls give the same bits whatever the device does beside them.  The cells, the domain and the fp64 weights are those of
// sn_hashgrid.h's backward_table, through the same cell policies (SnHgTorchGrid, SnHgTcnnGrid); DESIGN.md §4 "Ordered table gradient".
//
// One level at a time, M = 8 N contributions, contribution id c = 8 n + k (point n, corner slot k):
//   emit     one thread per point: vals[c] = fl32(w_k g_f) (F floats, the rounding the atomic form applies), keys[c] = the row within the
//            level, or SN_HGO_NONE for a point outside the domain.
//   sort     a stable LSD radix sort of (key, id), 8-bit digits, ceil(log2_T / 8) passes, ids implicit (= the position) in the first.
//            A key SN_HGO_NONE takes a bin of its own, 256, in EVERY pass, so those entries stay behind all rows at no extra pass.
//            Per pass: histogram (per workgroup tile of SN_HGO_TILE entries; LDS integer counters, whose totals no arrival order
//            changes), scan_digit (one workgroup per digit: an exclusive scan of that digit's counts over the tiles, and the digit's
//            total), scatter (the 257 totals are scanned in the workgroup; a wave owns SN_HGO_TILE / 4 consecutive entries and ranks them
//            with ballots, 64 at a time in position order; the waves' counts are chained through LDS).  Stable, so a row's entries end up in
//            ascending id order: the fixed order.
//   sum      one thread per sorted position.  The thread at a segment's head adds up to SN_HGO_SHORT entries one after another, in order.  A
//            longer segment goes to the whole wave: lane j adds the entries at j, j + 64, ... of the segment in order, then the 64 partial
//            sums are folded by a fixed tree (lane j takes lane j + d for d = 32, 16 .. 1).  Both are functions of the segment's length alone.
//            All sums are fp64; grad_table[r][f] = fl32((double)grad_table[r][f] + S), a plain store by the one thread that owns the row.
//
// Bounds.  M < 2^31 (the entry point refuses N >= 2^28), so positions, ids and their sums with a tile or a wave fit uint32.  scatter
// writes position p only if p < M (it always is when the counts are consistent; the guard is there for the machine's sake).
#pragma once
#include "sn_hashgrid.h"

#define SN_HGO_NONE 0xffffffffu
#define SN_HGO_BINS 257           // 256 digits and the bin of SN_HGO_NONE
#define SN_HGO_BLOCK 256
#define SN_HGO_WAVES 4
#define SN_HGO_ROUNDS 16          // a wave ranks 64 entries per round
#define SN_HGO_TILE (SN_HGO_BLOCK * SN_HGO_ROUNDS)
#define SN_HGO_SHORT 16

struct SnHgOrderedParams {
    SnHashgridParams g;
    float* vals;               // [M, F]
    const uint32_t* keys_in;   // [M]
    const uint32_t* ids_in;    // [M] (unused by the first pass)
    uint32_t* keys_out;        // [M] (emit writes here)
    uint32_t* ids_out;         // [M]
    uint32_t* hist;            // [SN_HGO_BINS, tiles]
    uint32_t* totals;          // [SN_HGO_BINS]
    uint32_t M, tiles;
    int32_t level, shift;
};

SN_DEV uint32_t sn_hgo_digit(uint32_t key, int shift) { return key == SN_HGO_NONE ? 256u : ((key >> shift) & 255u); }

// exclusive scan of one value per thread over the block of SN_HGO_BLOCK; *total is the block's sum.  Every thread calls it.
SN_DEV uint32_t sn_hgo_block_scan(uint32_t v, uint32_t* wave_sums /* LDS [SN_HGO_WAVES] */, uint32_t* total) {
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    __syncthreads();   // (the previous call's readers are done with wave_sums)
    if (lane == 63) wave_sums[w] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < SN_HGO_WAVES; ++i) {
        const uint32_t s = wave_sums[i];
        before += i < w ? s : 0u;
        all += s;
    }
    *total = all;
    return before + incl - v;
}

template <int F, class G>
__global__ __launch_bounds__(SN_HGO_BLOCK) void sn_hashgrid_ordered_emit_kernel(SnHgOrderedParams p) {
    const int64_t n = (int64_t)blockIdx.x * SN_HGO_BLOCK + threadIdx.x;
    if (n >= p.g.N) return;
    const float q[3] = {p.g.q[n * 3], p.g.q[n * 3 + 1], p.g.q[n * 3 + 2]};
    const int l = p.level;
    uint32_t* keys = p.keys_out + n * 8;
    if (!G::in_domain(q, p.g.scal, p.g.L)) {
        *reinterpret_cast<uint4*>(keys) = make_uint4(SN_HGO_NONE, SN_HGO_NONE, SN_HGO_NONE, SN_HGO_NONE);
        *reinterpret_cast<uint4*>(keys + 4) = make_uint4(SN_HGO_NONE, SN_HGO_NONE, SN_HGO_NONE, SN_HGO_NONE);
        return;   // (its vals are never read)
    }
    uint32_t row[8];
    float o[3];
    G::cell(q, p.g.scal[l], l, p.g.log2_T, row, o);
    const SnHgRow<F> g = sn_hg_load<F>(p.g.grad_enc + (n * p.g.L + l) * F);
    const double ox = o[0], oy = o[1], oz = o[2];
    const uint32_t mask = (1u << p.g.log2_T) - 1u;   // row[k] = l T + r, r < T
    float* vals = p.vals + n * (8 * F);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double w = (((G::XF >> k) & 1u) ? 1.0 - ox : ox) * (((G::YF >> k) & 1u) ? 1.0 - oy : oy) * (((G::ZF >> k) & 1u) ? 1.0 - oz : oz);
        SnHgRow<F> v;
#pragma unroll
        for (int f = 0; f < F; ++f) v.v[f] = (float)(w * (double)g.v[f]);
        sn_hg_store<F>(vals + k * F, v);
        row[k] &= mask;
    }
    *reinterpret_cast<uint4*>(keys) = make_uint4(row[0], row[1], row[2], row[3]);
    *reinterpret_cast<uint4*>(keys + 4) = make_uint4(row[4], row[5], row[6], row[7]);
}

// hist[d][tile] = the number of entries of the tile with digit d
__global__ __launch_bounds__(SN_HGO_BLOCK) void sn_hashgrid_ordered_histogram_kernel(SnHgOrderedParams p) {
    __shared__ uint32_t count[SN_HGO_BINS];
    for (uint32_t d = threadIdx.x; d < SN_HGO_BINS; d += SN_HGO_BLOCK) count[d] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * (uint32_t)SN_HGO_TILE;
#pragma unroll 4
    for (int r = 0; r < SN_HGO_ROUNDS; ++r) {
        const uint32_t i = first + (uint32_t)r * SN_HGO_BLOCK + threadIdx.x;
        if (i < p.M) atomicAdd(&count[sn_hgo_digit(p.keys_in[i], p.shift)], 1u);   // integer counts: the totals know no order
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < SN_HGO_BINS; d += SN_HGO_BLOCK) p.hist[(size_t)d * p.tiles + blockIdx.x] = count[d];
}

// one workgroup per digit: hist[d][.] becomes its exclusive scan over the tiles, totals[d] its sum
__global__ __launch_bounds__(SN_HGO_BLOCK) void sn_hashgrid_ordered_scan_digit_kernel(SnHgOrderedParams p) {
    __shared__ uint32_t wave_sums[SN_HGO_WAVES];
    uint32_t* row = p.hist + (size_t)blockIdx.x * p.tiles;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < p.tiles; base += SN_HGO_BLOCK) {   // block-uniform
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < p.tiles ? row[t] : 0u;
        uint32_t total;
        const uint32_t ex = sn_hgo_block_scan(v, wave_sums, &total);
        if (t < p.tiles) row[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) p.totals[blockIdx.x] = carry;
}

// out[rank] = in, rank = (entries of a smaller digit) + (entries of this digit at an earlier position)
template <bool FIRST>
__global__ __launch_bounds__(SN_HGO_BLOCK) void sn_hashgrid_ordered_scatter_kernel(SnHgOrderedParams p) {
    __shared__ uint32_t wave_sums[SN_HGO_WAVES];
    __shared__ uint32_t digit_base[SN_HGO_BINS];
    __shared__ uint32_t wave_count[SN_HGO_WAVES][SN_HGO_BINS];   // loop 1: a wave's count so far per digit; then: its first rank
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t d = threadIdx.x; d < SN_HGO_WAVES * SN_HGO_BINS; d += SN_HGO_BLOCK) (&wave_count[0][0])[d] = 0u;
    {
        uint32_t all;
        const uint32_t ex = sn_hgo_block_scan(p.totals[threadIdx.x], wave_sums, &all);   // digits 0..255
        digit_base[threadIdx.x] = ex;
        if (threadIdx.x == 0) digit_base[256] = all;
    }
    __syncthreads();
    const uint32_t first = blockIdx.x * (uint32_t)SN_HGO_TILE + (uint32_t)w * (SN_HGO_ROUNDS * 64u) + (uint32_t)lane;
    uint32_t key[SN_HGO_ROUNDS], rank[SN_HGO_ROUNDS];
#pragma unroll
    for (int r = 0; r < SN_HGO_ROUNDS; ++r) {
        const uint32_t i = first + (uint32_t)r * 64u;
        key[r] = i < p.M ? p.keys_in[i] : SN_HGO_NONE;
    }
#pragma unroll
    for (int r = 0; r < SN_HGO_ROUNDS; ++r) {
        const uint32_t i = first + (uint32_t)r * 64u;
        const bool live = i < p.M;
        const uint32_t d = sn_hgo_digit(key[r], p.shift);
        unsigned long long same = __ballot(live);   // the live lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < 9; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long has = __ballot(live && bit);
            same &= bit ? has : ~has;
        }
        // Every lane of a digit's group reads the wave's counter, then the group's first lane advances it, and the next round reads it
        // again.  What orders these: the accesses are volatile (the compiler keeps them, in program order), a wave issues its LDS
        // instructions in order and the LDS completes them in order, and the release / acquire fences at wavefront scope say so to the
        // compiler's memory model.  No other wave touches wave_count[w] before the __syncthreads below.
        volatile uint32_t* const counter = &wave_count[w][d];
        const uint32_t before = *counter;
        rank[r] = before + (uint32_t)__popcll(same & below);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (live && (same & below) == 0ull) *counter = before + (uint32_t)__popcll(same);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < SN_HGO_BINS; d += SN_HGO_BLOCK) {
        uint32_t run = digit_base[d] + p.hist[(size_t)d * p.tiles + blockIdx.x];
#pragma unroll
        for (int i = 0; i < SN_HGO_WAVES; ++i) {
            const uint32_t c = wave_count[i][d];
            wave_count[i][d] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SN_HGO_ROUNDS; ++r) {
        const uint32_t i = first + (uint32_t)r * 64u;
        if (i < p.M) {
            const uint32_t pos = wave_count[w][sn_hgo_digit(key[r], p.shift)] + rank[r];
            if (pos < p.M) {
                p.keys_out[pos] = key[r];
                p.ids_out[pos] = FIRST ? i : p.ids_in[i];
            }
        }
    }
}

// grad_table[l T + key][f] = fl32(grad_table + the fp64 sum of the key's segment in position order)
template <int F>
__global__ __launch_bounds__(SN_HGO_BLOCK) void sn_hashgrid_ordered_segment_sum_kernel(SnHgOrderedParams p) {
    const uint32_t i = blockIdx.x * (uint32_t)SN_HGO_BLOCK + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t key = i < p.M ? p.keys_in[i] : SN_HGO_NONE;
    const bool head = key != SN_HGO_NONE && (i == 0u || p.keys_in[i - 1u] != key);
    float* const level = p.g.grad_table + ((size_t)p.level << p.g.log2_T) * F;
    // longer than SN_HGO_SHORT: sorted keys, so the entry SN_HGO_SHORT places on decides it without walking the segment
    const bool wide = head && i + SN_HGO_SHORT < p.M && p.keys_in[i + SN_HGO_SHORT] == key;
    if (head && !wide) {
        double acc[F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = 0.0;
        uint32_t j = 0;
        for (; j < SN_HGO_SHORT; ++j) {
            const uint32_t t = i + j;
            if (t >= p.M || p.keys_in[t] != key) break;
            const SnHgRow<F> v = sn_hg_load<F>(p.vals + (size_t)p.ids_in[t] * F);
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] += (double)v.v[f];
        }
        float* dst = level + (size_t)key * F;
        SnHgRow<F> o = sn_hg_load<F>(dst);
#pragma unroll
        for (int f = 0; f < F; ++f) o.v[f] = (float)((double)o.v[f] + acc[f]);
        sn_hg_store<F>(dst, o);
    }
    // the segments longer than SN_HGO_SHORT whose heads sit in this wave, one after another, by the whole wave
    unsigned long long todo = __ballot(wide);
    while (todo) {   // wave-uniform
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint32_t start = __shfl(i, src, 64), k = __shfl(key, src, 64);
        double acc[F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = 0.0;
        for (uint32_t t = start + (uint32_t)lane;; t += 64u) {
            const bool in = t < p.M && p.keys_in[t] == k;
            if (in) {
                const SnHgRow<F> v = sn_hg_load<F>(p.vals + (size_t)p.ids_in[t] * F);
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] += (double)v.v[f];
            }
            if (!__all(in)) break;   // sorted keys: the segment ends inside these 64 positions
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] += __shfl_down(acc[f], d, 64);   // lane 0's tree is the fixed one; the others' sums are unused
        }
        if (lane == 0) {
            float* dst = level + (size_t)k * F;
            SnHgRow<F> o = sn_hg_load<F>(dst);
#pragma unroll
            for (int f = 0; f < F; ++f) o.v[f] = (float)((double)o.v[f] + acc[f]);
            sn_hg_store<F>(dst, o);
        }
    }
}
