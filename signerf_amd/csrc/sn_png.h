// sn_png.h -- the kernels of include/signerf_hip_png.h: a device uint8 image to the bytes of its .png file (DESIGN.md §4 "PNG encoding").
// Every decision about a byte is a call into sn_png_codes.h, the header the serial host reference (tests/c/png_encode.cpp) is built from.
//
//   sn_png_segment_deflate_kernel  one 64-lane workgroup (one wave) per segment of SN_PNG_SEGMENT_BYTES filtered bytes:
//       the filtered bytes are formed in LDS straight from the image (no filtered copy in HBM) with the segment's Adler sums;
//       per candidate distance the "byte equals byte - d" bits are packed into 64-bit words by __ballot, so a match length is a count of
//       trailing ones; the segment is walked 64 positions at a time: each lane takes the best (length, distance) of its position, the
//       greedy chain is resolved on uniform values (a jump per MATCH: the literal runs between are mask arithmetic), the histogram is LDS
//       integer atomics; the two codes are built with a lane-parallel minimum search over unique keys; the three block types are priced;
//       a second, identical walk emits: a wave prefix sum of the tokens' bit lengths, bits OR-ed into LDS words; the words go to the
//       segment's slot of the workspace with its byte count and CRC-32.
//   sn_png_finish_file_kernel      one workgroup: exclusive scan of the byte counts (64-bit, in passes of 1024), the stream's Adler-32 and
//       the IDAT CRC-32 from the per-segment values (both are order-free sums), the file's head and tail, its byte count.
//   sn_png_compact_bytes_kernel    one workgroup per segment: slot -> file at the scanned offset, in words of the destination.
// Integer arithmetic only; ordinary stores only.
#pragma once
#include <hip/hip_runtime.h>

#include "sn_png_codes.h"

struct SnPngParams {
    const uint8_t* image;
    uint32_t h, w, c, row_bytes, stride;   // stride = 1 + row_bytes: a filtered row
    uint32_t stream_bytes, nseg;
    uint8_t* slots;        // [nseg][SN_PNG_SLOT_STRIDE]
    uint32_t* seg_bytes;   // [nseg]
    uint32_t* seg_crc;     // [nseg]
    uint32_t* seg_adler;   // [nseg][2]
    uint64_t* seg_off;     // [nseg]
    uint8_t* file;
    uint64_t* file_bytes;
};

constexpr uint32_t SN_PNG_EQ_WORDS = SN_PNG_SEGMENT_BYTES / 64 + 6;   // zero words behind the last so a run may read 5 words on

__device__ inline uint32_t sn_png_wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ inline uint32_t sn_png_wave_min(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline uint32_t sn_png_wave_max(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}
__device__ inline uint32_t sn_png_wave_xor(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v ^= __shfl_xor(v, m);
    return v;
}
__device__ inline uint32_t sn_png_read_lane(uint32_t v, uint32_t lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane((int)lane));
}

// sn_png_build_lengths by the whole wave: the same keys, so the same two minima at every merge and the same tree.
__device__ inline void sn_png_build_lengths_wave(const uint32_t* counts, int n, uint8_t* lens, uint32_t* key, uint16_t* parent, uint32_t lane) {
    for (uint32_t r = 0;; ++r) {
        uint32_t mine = 0;
        for (int i = (int)lane; i < n; i += 64) {
            const uint32_t c = sn_png_scaled_count(counts[i], r);
            key[i] = c ? sn_png_node_key(c, (uint32_t)i) : SN_PNG_NO_NODE;
            lens[i] = c ? 1 : 0;
            mine += c ? 1 : 0;
        }
        int m = (int)sn_png_wave_sum(mine);
        __syncthreads();
        if (m == 0) return;
        if (m == 1) {
            if (lane == 0) {
                const uint32_t j = sn_png_second_symbol(key[0] != SN_PNG_NO_NODE);
                key[j] = sn_png_node_key(1, j);
                lens[j] = 1;
            }
            m = 2;
            __syncthreads();
        }
        int nn = n;
        for (int k = 0; k < m - 1; ++k) {
            uint32_t lo = SN_PNG_NO_NODE, lo2 = SN_PNG_NO_NODE;   // the lane's two smallest (node i belongs to lane i % 64)
            for (int i = (int)lane; i < nn; i += 64) {
                const uint32_t v = key[i];
                if (v < lo) { lo2 = lo; lo = v; }
                else if (v < lo2) lo2 = v;
            }
            const uint32_t ka = sn_png_wave_min(lo);
            const uint32_t a = sn_png_key_index(ka);
            const uint32_t kb = sn_png_wave_min((a & 63u) == lane ? lo2 : lo);
            const uint32_t b = sn_png_key_index(kb);
            if (lane == 0) {
                key[a] = key[b] = SN_PNG_NO_NODE;
                key[nn] = sn_png_node_key(sn_png_key_count(ka) + sn_png_key_count(kb), (uint32_t)nn);
                parent[a] = parent[b] = (uint16_t)nn;
            }
            ++nn;
            __syncthreads();
        }
        const uint32_t root = (uint32_t)nn - 1;
        uint32_t deepest = 0;
        for (int i = (int)lane; i < n; i += 64) {
            if (!lens[i]) continue;
            uint32_t d = 0;
            for (uint32_t x = (uint32_t)i; x != root; x = parent[x]) ++d;
            lens[i] = (uint8_t)(d > 255 ? 255 : d);
            deepest = d > deepest ? d : deepest;
        }
        deepest = sn_png_wave_max(deepest);
        __syncthreads();
        if (deepest <= (uint32_t)SN_PNG_MAX_BITS) return;
    }
}

// The tokens that start in the 64 positions [base, base + 64) of a segment of n bytes.  `entry` (uniform) is where the parse enters the
// chunk, relative to base; it may lie behind the chunk when a match covers it whole.  Returns through the references: the lane's taken
// length (0: literal) and candidate index, whether a token starts at the lane's position; `entry` becomes the next chunk's.
template <int C>
__device__ inline void sn_png_parse_chunk(const uint64_t (*eq)[SN_PNG_EQ_WORDS], uint32_t base, uint32_t n, uint32_t lane,
                                          uint32_t& entry, uint32_t& taken, uint32_t& k_best, bool& starts_here) {
    taken = 0;
    k_best = 0;
    starts_here = false;
    if (entry >= 64) {   // uniform
        entry -= 64;
        return;
    }
    const uint32_t pos = base + lane;
    uint32_t best = 0;
    if (pos < n) {
        const uint32_t cap = n - pos < SN_PNG_MAX_MATCH ? n - pos : SN_PNG_MAX_MATCH;
#pragma unroll
        for (int k = 0; k < sn_png_num_dists(C); ++k) sn_png_consider(sn_png_run_ones(eq[k], SN_PNG_EQ_WORDS, pos, cap), (uint32_t)k, best, k_best);
    }
    taken = sn_png_taken_len(best);
    const uint64_t match_mask = __ballot(taken != 0);
    uint64_t starts = 0;
    uint32_t q = entry;
    while (q < 64) {
        const uint64_t mm = match_mask >> q;
        if (!mm) {   // literals to the end of the chunk
            starts |= ~0ull << q;
            q = 64;
            break;
        }
        const uint32_t t = (uint32_t)__builtin_ctzll(mm);   // t literals, then a match at q + t < 64
        starts |= ((1ull << t) - 1) << q;
        starts |= 1ull << (q + t);
        q = sn_png_next_pos(q + t, sn_png_read_lane(taken, q + t));
    }
    entry = q - 64;
    starts_here = pos < n && ((starts >> lane) & 1ull);
}

template <int C>
__global__ __launch_bounds__(64) void sn_png_segment_deflate_kernel(SnPngParams p) {
    constexpr int ND = sn_png_num_dists(C);
    __shared__ uint32_t s_data32[SN_PNG_SEGMENT_BYTES / 4];
    __shared__ uint32_t s_out[SN_PNG_SLOT_STRIDE / 4];   // the segment's bytes; before they are written, the tree's work arrays
    __shared__ uint64_t s_eq[ND][SN_PNG_EQ_WORDS];
    __shared__ uint32_t s_hist[SN_PNG_NSYM];
    __shared__ uint8_t s_lens[SN_PNG_NSYM + 4];
    __shared__ uint16_t s_codes[SN_PNG_NSYM];
    __shared__ uint32_t s_work[32];
    const uint32_t lane = threadIdx.x, seg = blockIdx.x;
    const uint32_t g0 = seg * SN_PNG_SEGMENT_BYTES;
    const uint32_t n = p.stream_bytes - g0 < SN_PNG_SEGMENT_BYTES ? p.stream_bytes - g0 : SN_PNG_SEGMENT_BYTES;
    const bool last = seg == p.nseg - 1;
    const uint8_t* data = (const uint8_t*)s_data32;
    const uint32_t nchunks = (n + 63) / 64;

    // 1. the filtered bytes, 4 per lane and step, and the Adler sums of the segment
    uint32_t sum_a = 0, sum_b = 0;   // per lane at most 256 bytes: sum_b <= 256 * 255 * 16384 < 2^32
    for (uint32_t it = 0; it < SN_PNG_SEGMENT_BYTES / 256; ++it) {
        const uint32_t i0 = (it * 64 + lane) * 4;
        uint32_t word = 0;
        if (i0 < n) {
            uint32_t row = (g0 + i0) / p.stride, col = (g0 + i0) - row * p.stride;
            for (uint32_t k = 0; k < 4 && i0 + k < n; ++k) {
                const uint32_t v = sn_png_filtered_byte(p.image, p.row_bytes, row, col);
                word |= v << (8 * k);
                sum_a += v;
                sum_b += (n - (i0 + k)) * v;
                if (++col == p.stride) { col = 0; ++row; }
            }
        }
        s_data32[it * 64 + lane] = word;
    }
    sum_a = sn_png_wave_sum(sum_a) % SN_PNG_ADLER_MOD;
    sum_b = sn_png_wave_sum(sum_b % SN_PNG_ADLER_MOD) % SN_PNG_ADLER_MOD;
    if (lane == 0) {
        p.seg_adler[2 * seg] = sum_a;
        p.seg_adler[2 * seg + 1] = sum_b;
    }
    for (uint32_t i = lane; i < (uint32_t)SN_PNG_NSYM; i += 64) s_hist[i] = 0;
    __syncthreads();

    // 2. the equality bits of every candidate
    for (uint32_t j = 0; j < SN_PNG_EQ_WORDS; ++j) {
        const uint32_t pos = j * 64 + lane;
        const uint32_t b = pos < n ? data[pos] : 0;
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const uint32_t d = sn_png_dist(C, k);
            const bool in = pos < n && pos >= d;
            const uint64_t word = __ballot(in && b == data[in ? pos - d : 0]);
            if (lane == 0) s_eq[k][j] = word;
        }
    }
    __syncthreads();

    // 3. first walk: the histogram
    uint32_t entry = 0, taken, k_best;
    bool starts_here;
    for (uint32_t j = 0; j < nchunks; ++j) {
        sn_png_parse_chunk<C>(s_eq, j * 64, n, lane, entry, taken, k_best, starts_here);
        if (starts_here) {
            uint32_t sym, eb, ev;
            if (taken) {
                sn_png_len_symbol(taken, sym, eb, ev);
                atomicAdd(&s_hist[sym], 1u);
                sn_png_dist_symbol(sn_png_dist(C, (int)k_best), sym, eb, ev);
                atomicAdd(&s_hist[SN_PNG_NLIT + sym], 1u);
            } else {
                atomicAdd(&s_hist[data[j * 64 + lane]], 1u);
            }
        }
    }
    __syncthreads();
    if (lane == 0) s_hist[256] = 1;
    __syncthreads();

    // 4. the two codes, the prices, the choice
    uint32_t* key = s_out;
    uint16_t* parent = (uint16_t*)(s_out + 2 * SN_PNG_NLIT);
    sn_png_build_lengths_wave(s_hist, SN_PNG_NLIT, s_lens, key, parent, lane);
    __syncthreads();
    sn_png_build_lengths_wave(s_hist + SN_PNG_NLIT, SN_PNG_NDIST, s_lens + SN_PNG_NLIT, key, parent, lane);
    __syncthreads();
    uint32_t fixed_bits = 0, dyn_bits = 0, bytes;
    for (uint32_t i = lane; i < (uint32_t)SN_PNG_NSYM; i += 64) sn_png_symbol_cost(i, s_hist[i], s_lens[i], fixed_bits, dyn_bits);
    fixed_bits = sn_png_wave_sum(fixed_bits);
    dyn_bits = sn_png_wave_sum(dyn_bits);
    const int type = sn_png_choose_block(n, fixed_bits, dyn_bits, last, bytes);
    __syncthreads();
    for (uint32_t i = lane; i < SN_PNG_SLOT_STRIDE / 4; i += 64) s_out[i] = 0;
    if (lane == 0 && type != 0) {
        if (type == 1) {
            sn_png_fixed_code(s_lens, s_codes);
        } else {
            sn_png_canonical_codes(s_lens, SN_PNG_NLIT, s_codes, s_work);
            sn_png_canonical_codes(s_lens + SN_PNG_NLIT, SN_PNG_NDIST, s_codes + SN_PNG_NLIT, s_work);
        }
    }
    __syncthreads();

    // 5. the block
    uint8_t* out = (uint8_t*)s_out;
    if (type == 0) {
        if (lane == 0) sn_png_write_stored_header(out, n, last);
        for (uint32_t i = lane; i < n; i += 64) out[5 + i] = data[i];
    } else {
        SnPngBitSink sink{s_out, 0};
        if (lane == 0) sn_png_write_block_header(sink, type, last, s_lens);
        __syncthreads();
        uint32_t bitpos = type == 2 ? SN_PNG_DYN_HEADER_BITS : 3;
        entry = 0;
        for (uint32_t j = 0; j < nchunks; ++j) {
            sn_png_parse_chunk<C>(s_eq, j * 64, n, lane, entry, taken, k_best, starts_here);
            uint64_t bits = 0;
            uint32_t nbits = 0;
            if (starts_here) sn_png_token_bits(taken, taken ? sn_png_dist(C, (int)k_best) : data[j * 64 + lane], s_lens, s_codes, bits, nbits);
            uint32_t incl = nbits;   // inclusive prefix sum over the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if ((int)lane >= d) incl += o;
            }
            if (nbits) {
                const uint32_t at = bitpos + incl - nbits, w = at >> 5, s = at & 31;
                const uint64_t lo = bits << s;                       // bits < 2^48, s < 32: at most 79 bits
                const uint32_t hi = s ? (uint32_t)(bits >> (64 - s)) : 0;
                atomicOr(&s_out[w], (uint32_t)lo);
                if ((uint32_t)(lo >> 32)) atomicOr(&s_out[w + 1], (uint32_t)(lo >> 32));
                if (hi) atomicOr(&s_out[w + 2], hi);
            }
            bitpos += sn_png_read_lane(incl, 63);
        }
        __syncthreads();
        if (lane == 0) {
            sink.pos = bitpos;
            sn_png_write_block_end(sink, s_lens, s_codes, last);   // the count it returns is `bytes`: the price is exact
        }
    }
    __syncthreads();

    // 6. the slot, the byte count, the CRC-32 of the bytes (64 pieces, combined by length)
    uint32_t* slot = (uint32_t*)(p.slots + (uint64_t)seg * SN_PNG_SLOT_STRIDE);
    for (uint32_t i = lane; i < (bytes + 3) / 4; i += 64) slot[i] = s_out[i];
    // a lane's piece is an ODD number of words, so the 64 lanes read 64 different LDS banks at every step
    const uint32_t per = 4 * (((bytes + 255) / 256) | 1u);
    const uint32_t begin = lane * per < bytes ? lane * per : bytes, end = begin + per < bytes ? begin + per : bytes;
    uint32_t reg = 0xFFFFFFFFu;
    for (uint32_t i = begin; i < end; i += 4) {
        const uint32_t word = s_out[i >> 2];
        for (uint32_t k = 0; k < 4 && i + k < end; ++k) reg = sn_png_crc_step(reg, (uint8_t)(word >> (8 * k)));
    }
    const uint32_t crc = sn_png_wave_xor(end > begin ? sn_png_crc_shift(~reg, bytes - end) : 0u);
    if (lane == 0) {
        p.seg_bytes[seg] = bytes;
        p.seg_crc[seg] = crc;
    }
}

__global__ __launch_bounds__(1024) void sn_png_finish_file_kernel(SnPngParams p) {
    __shared__ uint64_t s_scan[1024];
    __shared__ uint32_t s_red[3][1024];
    const uint32_t tid = threadIdx.x;
    // exclusive scan of the byte counts, 1024 segments a pass
    uint64_t carry = 0;
    for (uint32_t base = 0; base < p.nseg; base += 1024) {
        const uint32_t i = base + tid;
        const uint64_t v = i < p.nseg ? p.seg_bytes[i] : 0;
        s_scan[tid] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const uint64_t o = tid >= d ? s_scan[tid - d] : 0;
            __syncthreads();
            s_scan[tid] += o;
            __syncthreads();
        }
        if (i < p.nseg) p.seg_off[i] = carry + s_scan[tid] - v;
        carry += s_scan[1023];
        __syncthreads();
    }
    const uint64_t total = carry;   // the segments' bytes
    // the order-free sums: Adler (a, b) mod 65521 and the CRC's xor
    uint64_t acc_a = 0, acc_b = 0;
    uint32_t crc = 0;
    for (uint32_t i = tid; i < p.nseg; i += 1024) {
        const uint64_t seg_end = (uint64_t)i * SN_PNG_SEGMENT_BYTES + sn_png_segment_len(p.stream_bytes, i);
        sn_png_adler_accumulate(p.seg_adler[2 * i], p.seg_adler[2 * i + 1], p.stream_bytes - seg_end, acc_a, acc_b);
        const uint64_t seg_file_end = p.seg_off[i] + p.seg_bytes[i];   // (seg_off[i] was written above by this same thread)
        crc ^= sn_png_crc_shift(p.seg_crc[i], total - seg_file_end + 4);
    }
    s_red[0][tid] = (uint32_t)acc_a;
    s_red[1][tid] = (uint32_t)acc_b;
    s_red[2][tid] = crc;
    __syncthreads();
    for (uint32_t d = 512; d >= 1; d >>= 1) {
        if (tid < d) {
            s_red[0][tid] = (s_red[0][tid] + s_red[0][tid + d]) % SN_PNG_ADLER_MOD;
            s_red[1][tid] = (s_red[1][tid] + s_red[1][tid + d]) % SN_PNG_ADLER_MOD;
            s_red[2][tid] ^= s_red[2][tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        uint8_t* f = p.file;
        sn_png_write_file_head(f, p.h, p.w, p.c, (uint32_t)(2 + total + 4));
        const uint32_t adler = sn_png_adler_of_sums(s_red[0][0], s_red[1][0], p.stream_bytes);
        uint8_t* tail = f + SN_PNG_IDAT_OFFSET + total;
        sn_png_put_be32(tail, adler);
        const uint32_t idat_crc = s_red[2][0] ^ sn_png_crc_shift(sn_png_crc32(f + 37, 6), total + 4) ^ sn_png_crc32(tail, 4);
        sn_png_write_file_tail(tail, adler, idat_crc);
        *p.file_bytes = SN_PNG_FILE_FRAME_BYTES + total;
    }
}

__global__ __launch_bounds__(256) void sn_png_compact_bytes_kernel(SnPngParams p) {
    const uint32_t seg = blockIdx.x;
    const uint8_t* slot = p.slots + (uint64_t)seg * SN_PNG_SLOT_STRIDE;
    uint8_t* dst = p.file + SN_PNG_IDAT_OFFSET + p.seg_off[seg];
    const uint32_t bytes = p.seg_bytes[seg];
    // bytes up to the destination's first word boundary, whole destination words (the slot's bytes sit at another alignment), the rest
    uint32_t head = (uint32_t)((0u - (uint32_t)(uintptr_t)dst) & 3u);
    head = head < bytes ? head : bytes;
    const uint32_t words = (bytes - head) / 4, tail = head + 4 * words;
    if (threadIdx.x < head) dst[threadIdx.x] = slot[threadIdx.x];
    uint32_t* dst32 = (uint32_t*)(dst + head);
    for (uint32_t i = threadIdx.x; i < words; i += 256) {
        const uint8_t* s = slot + head + 4 * i;
        dst32[i] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    }
    if (threadIdx.x < bytes - tail) dst[tail + threadIdx.x] = slot[tail + threadIdx.x];
}
