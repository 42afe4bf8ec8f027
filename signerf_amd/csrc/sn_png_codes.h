// sn_png_codes.h -- everything that decides a byte of a png_encoder="hip" file (include/signerf_hip_png.h, DESIGN.md §4 "PNG encoding").
// Plain C++17 without the HIP runtime: it compiles alone with g++ (tests/c/png_encode.cpp builds the serial reference encoder from it) and
// its functions carry SN_PNG_HD so the kernels of sn_png.h call the same copy.  No tables, no floating point, no recursion, and no
// function-local array that is indexed at run time (the callers hand in the work arrays: LDS on the device).
//
// The stream: zlib header 78 01, then one deflate block per SEGMENT of SN_PNG_SEGMENT_BYTES filtered bytes (row 0 filter 0, other rows
// filter 2 "Up"), each deflated on its own; a Huffman block that is not the stream's last is followed by an empty stored block that
// puts the next segment on a byte boundary; Adler-32 of the filtered bytes.  The matcher tries a fixed ordered list of distances.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SN_PNG_HD __host__ __device__ inline
#else
#define SN_PNG_HD inline
#endif

constexpr uint32_t SN_PNG_SEGMENT_BYTES = 16384;
constexpr uint32_t SN_PNG_SLOT_STRIDE = 16400;   // a segment's slot of the workspace: its worst case (stored: 5 + segment bytes), 16-aligned
constexpr uint32_t SN_PNG_MAX_DIM = 8192;
constexpr int SN_PNG_NLIT = 286, SN_PNG_NDIST = 30, SN_PNG_NSYM = SN_PNG_NLIT + SN_PNG_NDIST;
constexpr int SN_PNG_MAX_BITS = 15;
constexpr uint32_t SN_PNG_MIN_MATCH = 3, SN_PNG_MAX_MATCH = 258;
constexpr int SN_PNG_MAX_DISTS = 8;
constexpr uint32_t SN_PNG_DYN_HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + SN_PNG_NSYM * 4;   // 1338 with BFINAL and BTYPE
constexpr uint32_t SN_PNG_FILE_FRAME_BYTES = 63;   // signature 8, IHDR 25, IDAT length+tag 8, 78 01, Adler 4, IDAT CRC 4, IEND 12
constexpr uint32_t SN_PNG_IDAT_OFFSET = 43;        // first segment byte in the file
constexpr uint32_t SN_PNG_ADLER_MOD = 65521;
constexpr uint32_t SN_PNG_NO_NODE = 0xFFFFFFFFu;

// ---- the candidate distances, in the order ties are broken ------------------------------------------------------------------------------
// One channel: 1, 2, 3, 4.  Three: 1, 3, 6 (the same channel of the pixels before).
SN_PNG_HD constexpr int sn_png_num_dists(int channels) { return channels == 1 ? 4 : 3; }
SN_PNG_HD constexpr uint32_t sn_png_dist(int channels, int k) {
    return channels == 1 ? (uint32_t)(k + 1) : (k == 0 ? 1u : k == 1 ? 3u : 6u);
}

// ---- symbols ----------------------------------------------------------------------------------------------------------------------------
SN_PNG_HD uint32_t sn_png_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }   // v >= 1

// match length 3..258 -> literal/length symbol 257..285, number of extra bits, their value
SN_PNG_HD void sn_png_len_symbol(uint32_t len, uint32_t& sym, uint32_t& ebits, uint32_t& eval) {
    const uint32_t l = len - 3;
    if (len == 258) { sym = 285; ebits = 0; eval = 0; return; }
    if (l < 8) { sym = 257 + l; ebits = 0; eval = 0; return; }
    const uint32_t e = sn_png_log2(l) - 2;
    sym = 257 + 4 * (e + 1) + ((l >> e) & 3);
    ebits = e;
    eval = l & ((1u << e) - 1);
}
// distance 1..32768 -> distance symbol 0..29
SN_PNG_HD void sn_png_dist_symbol(uint32_t dist, uint32_t& sym, uint32_t& ebits, uint32_t& eval) {
    const uint32_t d = dist - 1;
    if (d < 4) { sym = d; ebits = 0; eval = 0; return; }
    const uint32_t e = sn_png_log2(d) - 1;
    sym = 2 * e + 2 + ((d >> e) & 1);
    ebits = e;
    eval = d & ((1u << e) - 1);
}
SN_PNG_HD uint32_t sn_png_lit_extra_bits(uint32_t sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }
SN_PNG_HD uint32_t sn_png_dist_extra_bits(uint32_t sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
SN_PNG_HD uint32_t sn_png_fixed_lit_len(uint32_t sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// ---- the matcher ------------------------------------------------------------------------------------------------------------------------
// s: the segment's n filtered bytes.  Length of the match at p with distance d: it reads nothing before s[0] and nothing at or after s[n].
SN_PNG_HD uint32_t sn_png_match_len(const uint8_t* s, uint32_t p, uint32_t n, uint32_t d) {
    if (p < d) return 0;
    const uint32_t cap = n - p < SN_PNG_MAX_MATCH ? n - p : SN_PNG_MAX_MATCH;
    uint32_t l = 0;
    while (l < cap && s[p + l] == s[p + l - d]) ++l;
    return l;
}
// The same number from packed "s[q] == s[q - d]" bits (bit q of w, 0 for q < d and q >= n): the run of ones from bit p, at most cap.
// w holds nwords words; the caller pads so that nwords covers every bit up to p + cap.
SN_PNG_HD uint32_t sn_png_run_ones(const uint64_t* w, uint32_t nwords, uint32_t p, uint32_t cap) {
    uint32_t wi = p >> 6;
    const uint32_t s = p & 63;
    const uint64_t x = ~(w[wi] >> s);
    uint32_t avail = 64 - s;
    uint32_t run = x ? (uint32_t)__builtin_ctzll(x) : 64;
    if (run > avail) run = avail;
    while (run == avail && run < cap && ++wi < nwords) {
        const uint64_t y = ~w[wi];
        run += y ? (uint32_t)__builtin_ctzll(y) : 64;
        avail += 64;
    }
    return run < cap ? run : cap;
}
// One candidate after another: the longest wins, a tie keeps the earlier entry.  (len, index) start as (0, 0).
SN_PNG_HD void sn_png_consider(uint32_t len, uint32_t k, uint32_t& best_len, uint32_t& best_k) {
    if (len > best_len) { best_len = len; best_k = k; }
}
// What the greedy parser takes at p: a match when the best is long enough, else the literal.
SN_PNG_HD uint32_t sn_png_taken_len(uint32_t best_len) { return best_len >= SN_PNG_MIN_MATCH ? best_len : 0; }
SN_PNG_HD uint32_t sn_png_next_pos(uint32_t p, uint32_t taken_len) { return p + (taken_len ? taken_len : 1); }

template <int C>
SN_PNG_HD void sn_png_best_match(const uint8_t* s, uint32_t p, uint32_t n, uint32_t& len, uint32_t& k_best) {
    len = 0;
    k_best = 0;
    for (int k = 0; k < sn_png_num_dists(C); ++k) sn_png_consider(sn_png_match_len(s, p, n, sn_png_dist(C, k)), (uint32_t)k, len, k_best);
    len = sn_png_taken_len(len);
}

// ---- code lengths -----------------------------------------------------------------------------------------------------------------------
// A node's key orders the merge: by count, then by node index (leaves are 0..n-1, the k-th merged node is n + k).  Keys are unique, so the
// minimum does not depend on the order it is searched in.  Counts sum to less than 2^22, n <= 512.
SN_PNG_HD uint32_t sn_png_node_key(uint32_t count, uint32_t index) { return (count << 10) | index; }
SN_PNG_HD uint32_t sn_png_key_count(uint32_t key) { return key >> 10; }
SN_PNG_HD uint32_t sn_png_key_index(uint32_t key) { return key & 1023u; }
// the count a symbol enters round r with: halved r times, rounding up, never to 0
SN_PNG_HD uint32_t sn_png_scaled_count(uint32_t count, uint32_t r) { return count ? (count + (1u << r) - 1) >> r : 0; }
// with one used symbol a second one joins so that the code is complete: symbol 0, or symbol 1 when 0 is the used one
SN_PNG_HD uint32_t sn_png_second_symbol(bool symbol0_used) { return symbol0_used ? 1u : 0u; }

// Serial build.  key, parent: work arrays of 2 n entries.  lens[i] = 0 for an unused symbol.  No used symbol: all 0.
SN_PNG_HD void sn_png_build_lengths(const uint32_t* counts, int n, uint8_t* lens, uint32_t* key, uint16_t* parent) {
    for (uint32_t r = 0;; ++r) {
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const uint32_t c = sn_png_scaled_count(counts[i], r);
            key[i] = c ? sn_png_node_key(c, (uint32_t)i) : SN_PNG_NO_NODE;
            lens[i] = c ? 1 : 0;
            m += c ? 1 : 0;
        }
        if (m == 0) return;
        if (m == 1) {
            const uint32_t j = sn_png_second_symbol(key[0] != SN_PNG_NO_NODE);
            key[j] = sn_png_node_key(1, j);
            lens[j] = 1;
            m = 2;
        }
        int nn = n;
        for (int k = 0; k < m - 1; ++k) {
            uint32_t ka = SN_PNG_NO_NODE, kb = SN_PNG_NO_NODE;
            for (int i = 0; i < nn; ++i) {
                const uint32_t v = key[i];
                if (v < ka) { kb = ka; ka = v; }
                else if (v < kb) kb = v;
            }
            const uint32_t a = sn_png_key_index(ka), b = sn_png_key_index(kb);
            key[a] = key[b] = SN_PNG_NO_NODE;
            key[nn] = sn_png_node_key(sn_png_key_count(ka) + sn_png_key_count(kb), (uint32_t)nn);
            parent[a] = parent[b] = (uint16_t)nn;
            ++nn;
        }
        const uint32_t root = (uint32_t)nn - 1;
        uint32_t deepest = 0;
        for (int i = 0; i < n; ++i) {
            if (!lens[i]) continue;
            uint32_t d = 0;
            for (uint32_t x = (uint32_t)i; x != root; x = parent[x]) ++d;
            lens[i] = (uint8_t)(d > 255 ? 255 : d);
            if (d > deepest) deepest = d;
        }
        if (deepest <= (uint32_t)SN_PNG_MAX_BITS) return;
    }
}

SN_PNG_HD uint32_t sn_png_reverse_bits(uint32_t v, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}
// Canonical codes of the lengths, already bit-reversed (deflate sends a code from its most significant bit).  work: 32 entries.
SN_PNG_HD void sn_png_canonical_codes(const uint8_t* lens, int n, uint16_t* codes, uint32_t* work) {
    uint32_t* count = work;
    uint32_t* next = work + 16;
    for (int b = 0; b < 16; ++b) count[b] = 0;
    for (int i = 0; i < n; ++i) count[lens[i]]++;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (int i = 0; i < n; ++i) {
        const uint32_t l = lens[i];
        codes[i] = l ? (uint16_t)sn_png_reverse_bits(next[l]++, l) : 0;
    }
}
// The fixed block's lengths and (bit-reversed) codes.  They are the canonical codes of 288 + 32 symbols, of which a block may use 286 + 30.
SN_PNG_HD uint32_t sn_png_fixed_lit_code(uint32_t sym) { return sym < 144 ? 0x30 + sym : sym < 256 ? 0x190 + (sym - 144) : sym < 280 ? sym - 256 : 0xC0 + (sym - 280); }
SN_PNG_HD void sn_png_fixed_code(uint8_t* lens, uint16_t* codes /* [SN_PNG_NSYM]: literal/length, then distance */) {
    for (int s = 0; s < SN_PNG_NLIT; ++s) {
        lens[s] = (uint8_t)sn_png_fixed_lit_len((uint32_t)s);
        codes[s] = (uint16_t)sn_png_reverse_bits(sn_png_fixed_lit_code((uint32_t)s), lens[s]);
    }
    for (int d = 0; d < SN_PNG_NDIST; ++d) {
        lens[SN_PNG_NLIT + d] = 5;
        codes[SN_PNG_NLIT + d] = (uint16_t)sn_png_reverse_bits((uint32_t)d, 5);
    }
}

// ---- cost and choice --------------------------------------------------------------------------------------------------------------------
// A symbol's share of the two Huffman blocks' token bits (hist: [SN_PNG_NSYM], literal/length then distance, EOB counted once).
SN_PNG_HD void sn_png_symbol_cost(uint32_t s, uint32_t count, uint32_t dyn_len, uint32_t& fixed_bits, uint32_t& dyn_bits) {
    const bool lit = s < (uint32_t)SN_PNG_NLIT;
    const uint32_t extra = lit ? sn_png_lit_extra_bits(s) : sn_png_dist_extra_bits(s - SN_PNG_NLIT);
    fixed_bits += count * ((lit ? sn_png_fixed_lit_len(s) : 5u) + extra);
    dyn_bits += count * (dyn_len + extra);
}
// The exact bit count of a segment's block: a stored block starts on a byte boundary, so it is 3 bits, 5 of padding, LEN, NLEN and the
// bytes; a Huffman block is its `bits` (header and EOB included) and, when it is not the stream's last, the 3 + 32 bits of the empty
// stored block behind it (BFINAL/BTYPE and 00 00 FF FF; the padding between them, which depends on where the block ends, is not counted).
SN_PNG_HD uint32_t sn_png_stored_bits(uint32_t n) { return 3 + 5 + 32 + 8 * n; }
SN_PNG_HD uint32_t sn_png_huffman_bits(uint32_t bits, bool last) { return last ? bits : bits + 3 + 32; }
// Bytes the segment then occupies.  A Huffman block is chosen only below the stored count, so no segment exceeds 5 + n bytes:
// bits + 35 < 40 + 8 n gives (bits + 3 + 7) / 8 + 4 <= n + 5, and for the last block bits < 40 + 8 n gives (bits + 7) / 8 <= n + 5.
SN_PNG_HD uint32_t sn_png_stored_bytes(uint32_t n) { return 5 + n; }
SN_PNG_HD uint32_t sn_png_huffman_bytes(uint32_t bits, bool last) { return last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4; }
// BTYPE of the cheapest by exact bit count; ties go to the lower BTYPE.  token bits exclude the block headers.
SN_PNG_HD int sn_png_choose_block(uint32_t n, uint32_t fixed_token_bits, uint32_t dyn_token_bits, bool last, uint32_t& bytes) {
    const uint32_t f = 3 + fixed_token_bits, d = SN_PNG_DYN_HEADER_BITS + dyn_token_bits;
    int type = 0;
    uint32_t best = sn_png_stored_bits(n);
    if (sn_png_huffman_bits(f, last) < best) { type = 1; best = sn_png_huffman_bits(f, last); }
    if (sn_png_huffman_bits(d, last) < best) { type = 2; best = sn_png_huffman_bits(d, last); }
    bytes = type == 0 ? sn_png_stored_bytes(n) : sn_png_huffman_bytes(type == 1 ? f : d, last);
    return type;
}

// ---- writing ----------------------------------------------------------------------------------------------------------------------------
// Bits go into 32-bit little-endian words from the least significant bit, as deflate packs them.  The words start zeroed.
struct SnPngBitSink {
    uint32_t* words;
    uint32_t pos;   // in bits
    SN_PNG_HD void put(uint32_t value, uint32_t nbits) {   // nbits <= 32, value < 2^nbits
        if (!nbits) return;
        const uint32_t w = pos >> 5, s = pos & 31;
        words[w] |= value << s;
        if (s + nbits > 32) words[w + 1] |= value >> (32 - s);
        pos += nbits;
    }
    SN_PNG_HD void align() { pos = (pos + 7) & ~7u; }
};
// BFINAL, BTYPE and, for a dynamic block, the code lengths: HLIT = 286, HDIST = 30, HCLEN = 19, a code-length code of 4 bits for the
// symbols 0..15 and none for the repeat symbols 16, 17, 18 (sent first in deflate's order), in which a symbol's code is its own value.
SN_PNG_HD void sn_png_write_block_header(SnPngBitSink& out, int type, bool final, const uint8_t* lens /* [SN_PNG_NSYM] */) {
    out.put(final ? 1u : 0u, 1);
    out.put((uint32_t)type, 2);
    if (type != 2) return;
    out.put(SN_PNG_NLIT - 257, 5);
    out.put(SN_PNG_NDIST - 1, 5);
    out.put(19 - 4, 4);
    for (int k = 0; k < 19; ++k) out.put(k < 3 ? 0u : 4u, 3);
    for (int s = 0; s < SN_PNG_NSYM; ++s) out.put(sn_png_reverse_bits(lens[s], 4), 4);
}
SN_PNG_HD void sn_png_write_stored_header(uint8_t* out, uint32_t n, bool final) {
    out[0] = final ? 1 : 0;
    out[1] = (uint8_t)(n & 255);
    out[2] = (uint8_t)(n >> 8);
    out[3] = (uint8_t)(~n & 255);
    out[4] = (uint8_t)((~n >> 8) & 255);
}
// EOB and what follows the tokens of a Huffman block; returns the segment's byte count.
SN_PNG_HD uint32_t sn_png_write_block_end(SnPngBitSink& out, const uint8_t* lens, const uint16_t* codes, bool last) {
    out.put(codes[256], lens[256]);
    if (!last) {
        out.put(0, 3);
        out.align();
        out.put(0xFFFF0000u, 32);
    }
    out.align();
    return out.pos >> 3;
}
// The bits of one token: a literal (taken_len = 0, value = the byte) or a match.  At most 48 bits.
SN_PNG_HD void sn_png_token_bits(uint32_t taken_len, uint32_t value_or_dist, const uint8_t* lens, const uint16_t* codes, uint64_t& bits,
                                 uint32_t& nbits) {
    if (!taken_len) {
        bits = codes[value_or_dist];
        nbits = lens[value_or_dist];
        return;
    }
    uint32_t sym, eb, ev, dsym, deb, dev;
    sn_png_len_symbol(taken_len, sym, eb, ev);
    sn_png_dist_symbol(value_or_dist, dsym, deb, dev);
    dsym += SN_PNG_NLIT;
    bits = codes[sym];
    nbits = lens[sym];
    bits |= (uint64_t)ev << nbits;
    nbits += eb;
    bits |= (uint64_t)codes[dsym] << nbits;
    nbits += lens[dsym];
    bits |= (uint64_t)dev << nbits;
    nbits += deb;
}

// ---- the filtered stream and the segment plan -------------------------------------------------------------------------------------------
SN_PNG_HD bool sn_png_shape_ok(int64_t h, int64_t w, int64_t c) {
    return (c == 1 || c == 3) && h >= 1 && h <= (int64_t)SN_PNG_MAX_DIM && w >= 1 && w <= (int64_t)SN_PNG_MAX_DIM;
}
SN_PNG_HD uint64_t sn_png_stream_bytes(uint32_t h, uint32_t w, uint32_t c) { return (uint64_t)h * (1 + (uint64_t)w * c); }   // < 2^28
SN_PNG_HD uint32_t sn_png_segment_count(uint64_t stream_bytes) { return (uint32_t)((stream_bytes + SN_PNG_SEGMENT_BYTES - 1) / SN_PNG_SEGMENT_BYTES); }
SN_PNG_HD uint32_t sn_png_segment_len(uint64_t stream_bytes, uint32_t seg) {
    const uint64_t left = stream_bytes - (uint64_t)seg * SN_PNG_SEGMENT_BYTES;
    return left < SN_PNG_SEGMENT_BYTES ? (uint32_t)left : SN_PNG_SEGMENT_BYTES;
}
// every segment stored: the exact upper bound of a file
SN_PNG_HD uint64_t sn_png_file_bound(uint32_t h, uint32_t w, uint32_t c) {
    const uint64_t n = sn_png_stream_bytes(h, w, c);
    return SN_PNG_FILE_FRAME_BYTES + n + 5ull * sn_png_segment_count(n);
}
// workspace: the slots, then per segment the offset as uint64 and bytes, CRC, Adler sums (2) as uint32
SN_PNG_HD uint64_t sn_png_workspace_size(uint32_t h, uint32_t w, uint32_t c) {
    return (uint64_t)sn_png_segment_count(sn_png_stream_bytes(h, w, c)) * (SN_PNG_SLOT_STRIDE + 4 * 4 + 8);
}
// byte g of the filtered stream, from the image (row_bytes = w * c)
SN_PNG_HD uint8_t sn_png_filtered_byte(const uint8_t* image, uint32_t row_bytes, uint32_t row, uint32_t col /* 0 = the filter byte */) {
    if (col == 0) return row ? 2 : 0;
    const uint8_t v = image[(uint64_t)row * row_bytes + col - 1];
    return row ? (uint8_t)(v - image[(uint64_t)(row - 1) * row_bytes + col - 1]) : v;
}

// ---- Adler-32 ---------------------------------------------------------------------------------------------------------------------------
// A piece of n bytes is kept as (sum of bytes, sum of (n - i) * byte i), both mod 65521; its Adler-32 starts from a = 1.
SN_PNG_HD uint32_t sn_png_adler_of_sums(uint32_t sum_a, uint32_t sum_b, uint64_t n) {
    return ((uint32_t)((n + sum_b) % SN_PNG_ADLER_MOD) << 16) | ((1 + sum_a) % SN_PNG_ADLER_MOD);
}
// what a piece adds to the whole's two sums when suffix_len bytes follow it
SN_PNG_HD void sn_png_adler_accumulate(uint32_t sum_a, uint32_t sum_b, uint64_t suffix_len, uint64_t& acc_a, uint64_t& acc_b) {
    acc_a = (acc_a + sum_a) % SN_PNG_ADLER_MOD;
    acc_b = (acc_b + sum_b + (suffix_len % SN_PNG_ADLER_MOD) * sum_a) % SN_PNG_ADLER_MOD;
}
// Adler-32 of A || B from Adler-32(A), Adler-32(B) and B's length
SN_PNG_HD uint32_t sn_png_adler_combine(uint32_t adler1, uint32_t adler2, uint64_t len2) {
    const uint64_t M = SN_PNG_ADLER_MOD, rem = len2 % M, a1 = adler1 & 0xffff, b1 = adler1 >> 16, a2 = adler2 & 0xffff, b2 = adler2 >> 16;
    const uint64_t a = (a1 + a2 + M - 1) % M, b = (rem * a1 + b1 + b2 + M - rem) % M;
    return (uint32_t)((b << 16) | a);
}

// ---- CRC-32 -----------------------------------------------------------------------------------------------------------------------------
SN_PNG_HD uint32_t sn_png_crc_step(uint32_t reg, uint8_t byte) {   // reg: the inverted register
    reg ^= byte;
    for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (0xEDB88320u & (0u - (reg & 1u)));
    return reg;
}
SN_PNG_HD uint32_t sn_png_crc32(const uint8_t* s, uint64_t n) {
    uint32_t reg = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; ++i) reg = sn_png_crc_step(reg, s[i]);
    return ~reg;
}
// product of two polynomials mod the CRC polynomial, bit 31 = x^0
SN_PNG_HD uint32_t sn_png_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
    }
    return p;
}
SN_PNG_HD uint32_t sn_png_crc_xpow8(uint64_t len) {   // x^(8 len)
    uint32_t p = 0x80000000u, sq = 0x00800000u;
    for (; len; len >>= 1) {
        if (len & 1) p = sn_png_crc_mul(sq, p);
        sq = sn_png_crc_mul(sq, sq);
    }
    return p;
}
// what the CRC-32 of a piece adds (by xor) to the CRC-32 of the whole when suffix_len bytes follow it
SN_PNG_HD uint32_t sn_png_crc_shift(uint32_t crc, uint64_t suffix_len) { return sn_png_crc_mul(sn_png_crc_xpow8(suffix_len), crc); }
SN_PNG_HD uint32_t sn_png_crc_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) { return sn_png_crc_shift(crc1, len2) ^ crc2; }

// ---- the file's frame -------------------------------------------------------------------------------------------------------------------
SN_PNG_HD void sn_png_put_be32(uint8_t* out, uint32_t v) {
    out[0] = (uint8_t)(v >> 24);
    out[1] = (uint8_t)(v >> 16);
    out[2] = (uint8_t)(v >> 8);
    out[3] = (uint8_t)v;
}
// the 43 bytes before the first segment; payload_bytes = 2 + the segments' bytes + 4
SN_PNG_HD void sn_png_write_file_head(uint8_t* f, uint32_t h, uint32_t w, uint32_t c, uint32_t payload_bytes) {
    f[0] = 0x89; f[1] = 'P'; f[2] = 'N'; f[3] = 'G'; f[4] = 13; f[5] = 10; f[6] = 26; f[7] = 10;
    sn_png_put_be32(f + 8, 13);
    f[12] = 'I'; f[13] = 'H'; f[14] = 'D'; f[15] = 'R';
    sn_png_put_be32(f + 16, w);
    sn_png_put_be32(f + 20, h);
    f[24] = 8; f[25] = c == 1 ? 0 : 2; f[26] = 0; f[27] = 0; f[28] = 0;
    sn_png_put_be32(f + 29, sn_png_crc32(f + 12, 17));
    sn_png_put_be32(f + 33, payload_bytes);
    f[37] = 'I'; f[38] = 'D'; f[39] = 'A'; f[40] = 'T'; f[41] = 0x78; f[42] = 0x01;
}
// the 20 bytes after the last segment
SN_PNG_HD void sn_png_write_file_tail(uint8_t* f, uint32_t adler, uint32_t idat_crc) {
    sn_png_put_be32(f, adler);
    sn_png_put_be32(f + 4, idat_crc);
    sn_png_put_be32(f + 8, 0);
    f[12] = 'I'; f[13] = 'E'; f[14] = 'N'; f[15] = 'D';
    sn_png_put_be32(f + 16, 0xAE426082u);
}
