// The serial host reference encoder of png_encoder="hip", built from signerf_amd/csrc/sn_png_codes.h alone (no HIP, no zlib): uint8 pixels
// in, a complete .png file out.  The kernels of sn_png.h must produce the same bytes.
//   png_encode encode H W C pixels.raw out.png [bits]   "bits": match lengths from the packed equality bits, as the kernel takes them
//   png_encode plan H W C                               segment bytes, segment count, file bound, workspace bytes
//   png_encode lengths c0 c1 ...                        code lengths of these counts, then the deepest and the Kraft sum * 2^15
//   png_encode sums file cut1 cut2                      CRC-32 and Adler-32 of a file from 3 pieces, combined
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../signerf_amd/csrc/sn_png_codes.h"

static std::vector<uint8_t> read_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

struct Matcher {
    const uint8_t* s;
    uint32_t n;
    bool bits;
    std::vector<std::vector<uint64_t>> eq;   // per candidate
    template <int C>
    void prepare() {
        if (!bits) return;
        const uint32_t nwords = SN_PNG_SEGMENT_BYTES / 64 + 6;
        eq.assign(sn_png_num_dists(C), std::vector<uint64_t>(nwords, 0));
        for (int k = 0; k < sn_png_num_dists(C); ++k) {
            const uint32_t d = sn_png_dist(C, k);
            for (uint32_t q = d; q < n; ++q)
                if (s[q] == s[q - d]) eq[k][q >> 6] |= 1ull << (q & 63);
        }
    }
    template <int C>
    void best(uint32_t p, uint32_t& len, uint32_t& k_best) const {
        if (!bits) return sn_png_best_match<C>(s, p, n, len, k_best);
        len = 0;
        k_best = 0;
        const uint32_t cap = n - p < SN_PNG_MAX_MATCH ? n - p : SN_PNG_MAX_MATCH;
        for (int k = 0; k < sn_png_num_dists(C); ++k)
            sn_png_consider(sn_png_run_ones(eq[k].data(), (uint32_t)eq[k].size(), p, cap), (uint32_t)k, len, k_best);
        len = sn_png_taken_len(len);
    }
};

// one segment: n filtered bytes -> its bytes of the stream
template <int C>
static std::vector<uint8_t> encode_segment(const uint8_t* s, uint32_t n, bool last, bool bits) {
    Matcher m{s, n, bits, {}};
    m.prepare<C>();
    std::vector<uint32_t> hist(SN_PNG_NSYM, 0);
    uint32_t len, k, sym, eb, ev;
    for (uint32_t p = 0; p < n; p = sn_png_next_pos(p, len)) {
        m.best<C>(p, len, k);
        if (len) {
            sn_png_len_symbol(len, sym, eb, ev);
            hist[sym]++;
            sn_png_dist_symbol(sn_png_dist(C, (int)k), sym, eb, ev);
            hist[SN_PNG_NLIT + sym]++;
        } else {
            hist[s[p]]++;
        }
    }
    hist[256] = 1;
    std::vector<uint8_t> lens(SN_PNG_NSYM + 4, 0);
    std::vector<uint32_t> key(2 * SN_PNG_NLIT);
    std::vector<uint16_t> parent(2 * SN_PNG_NLIT);
    sn_png_build_lengths(hist.data(), SN_PNG_NLIT, lens.data(), key.data(), parent.data());
    sn_png_build_lengths(hist.data() + SN_PNG_NLIT, SN_PNG_NDIST, lens.data() + SN_PNG_NLIT, key.data(), parent.data());
    uint32_t fixed_bits = 0, dyn_bits = 0, bytes;
    for (uint32_t i = 0; i < (uint32_t)SN_PNG_NSYM; ++i) sn_png_symbol_cost(i, hist[i], lens[i], fixed_bits, dyn_bits);
    const int type = sn_png_choose_block(n, fixed_bits, dyn_bits, last, bytes);
    std::vector<uint32_t> words(SN_PNG_SLOT_STRIDE / 4, 0);
    uint8_t* out = (uint8_t*)words.data();
    if (type == 0) {
        sn_png_write_stored_header(out, n, last);
        memcpy(out + 5, s, n);
        return std::vector<uint8_t>(out, out + bytes);
    }
    std::vector<uint16_t> codes(SN_PNG_NSYM);
    uint32_t work[32];
    if (type == 1) {
        sn_png_fixed_code(lens.data(), codes.data());
    } else {
        sn_png_canonical_codes(lens.data(), SN_PNG_NLIT, codes.data(), work);
        sn_png_canonical_codes(lens.data() + SN_PNG_NLIT, SN_PNG_NDIST, codes.data() + SN_PNG_NLIT, work);
    }
    SnPngBitSink sink{words.data(), 0};
    sn_png_write_block_header(sink, type, last, lens.data());
    for (uint32_t p = 0; p < n; p = sn_png_next_pos(p, len)) {
        m.best<C>(p, len, k);
        uint64_t b;
        uint32_t nb;
        sn_png_token_bits(len, len ? sn_png_dist(C, (int)k) : s[p], lens.data(), codes.data(), b, nb);
        sink.put((uint32_t)b, nb < 32 ? nb : 32);
        if (nb > 32) sink.put((uint32_t)(b >> 32), nb - 32);
    }
    const uint32_t got = sn_png_write_block_end(sink, lens.data(), codes.data(), last);
    if (got != bytes) { fprintf(stderr, "segment of %u bytes: priced %u bytes, wrote %u\n", n, bytes, got); exit(3); }
    return std::vector<uint8_t>(out, out + bytes);
}

static std::vector<uint8_t> encode(const std::vector<uint8_t>& px, uint32_t h, uint32_t w, uint32_t c, bool bits) {
    const uint64_t total = sn_png_stream_bytes(h, w, c);
    const uint32_t stride = 1 + w * c, nseg = sn_png_segment_count(total);
    std::vector<uint8_t> stream(total);
    for (uint32_t r = 0; r < h; ++r)
        for (uint32_t k = 0; k < stride; ++k) stream[(uint64_t)r * stride + k] = sn_png_filtered_byte(px.data(), w * c, r, k);
    std::vector<uint8_t> file(SN_PNG_IDAT_OFFSET);
    uint64_t acc_a = 0, acc_b = 0;
    std::vector<uint32_t> crcs;
    std::vector<uint64_t> sizes;
    for (uint32_t i = 0; i < nseg; ++i) {
        const uint32_t n = sn_png_segment_len(total, i);
        const uint8_t* s = stream.data() + (uint64_t)i * SN_PNG_SEGMENT_BYTES;
        const std::vector<uint8_t> seg = c == 1 ? encode_segment<1>(s, n, i == nseg - 1, bits) : encode_segment<3>(s, n, i == nseg - 1, bits);
        uint32_t sa = 0, sb = 0;
        for (uint32_t j = 0; j < n; ++j) {
            sa = (sa + s[j]) % SN_PNG_ADLER_MOD;
            sb = (uint32_t)((sb + (uint64_t)(n - j) * s[j]) % SN_PNG_ADLER_MOD);
        }
        sn_png_adler_accumulate(sa, sb, total - ((uint64_t)i * SN_PNG_SEGMENT_BYTES + n), acc_a, acc_b);
        crcs.push_back(sn_png_crc32(seg.data(), seg.size()));
        sizes.push_back(seg.size());
        file.insert(file.end(), seg.begin(), seg.end());
    }
    const uint64_t seg_total = file.size() - SN_PNG_IDAT_OFFSET;
    sn_png_write_file_head(file.data(), h, w, c, (uint32_t)(2 + seg_total + 4));
    const uint32_t adler = sn_png_adler_of_sums((uint32_t)acc_a, (uint32_t)acc_b, total);
    // the IDAT CRC from the pieces' CRCs, as the finish kernel combines them
    uint32_t crc = sn_png_crc_shift(sn_png_crc32(file.data() + 37, 6), seg_total + 4);
    uint64_t off = 0;
    for (uint32_t i = 0; i < nseg; ++i) {
        off += sizes[i];
        crc ^= sn_png_crc_shift(crcs[i], seg_total - off + 4);
    }
    uint8_t tail[20];
    sn_png_put_be32(tail, adler);
    crc ^= sn_png_crc32(tail, 4);
    sn_png_write_file_tail(tail, adler, crc);
    file.insert(file.end(), tail, tail + 20);
    if (file.size() > sn_png_file_bound(h, w, c)) { fprintf(stderr, "file exceeds its bound\n"); exit(3); }
    return file;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "encode" && argc >= 7) {
        const long h = atol(argv[2]), w = atol(argv[3]), c = atol(argv[4]);
        if (!sn_png_shape_ok(h, w, c)) { fprintf(stderr, "refused shape\n"); return 1; }
        const std::vector<uint8_t> px = read_file(argv[5]);
        if (px.size() != (size_t)h * w * c) { fprintf(stderr, "%zu pixels bytes for %ldx%ldx%ld\n", px.size(), h, w, c); return 1; }
        const std::vector<uint8_t> file = encode(px, (uint32_t)h, (uint32_t)w, (uint32_t)c, argc > 7 && std::string(argv[7]) == "bits");
        FILE* f = fopen(argv[6], "wb");
        if (!f || fwrite(file.data(), 1, file.size(), f) != file.size()) { fprintf(stderr, "cannot write %s\n", argv[6]); return 2; }
        fclose(f);
        return 0;
    }
    if (cmd == "plan" && argc == 5) {
        const long h = atol(argv[2]), w = atol(argv[3]), c = atol(argv[4]);
        if (!sn_png_shape_ok(h, w, c)) { printf("%u 0 0 0\n", SN_PNG_SEGMENT_BYTES); return 0; }
        printf("%u %u %llu %llu\n", SN_PNG_SEGMENT_BYTES, sn_png_segment_count(sn_png_stream_bytes(h, w, c)),
               (unsigned long long)sn_png_file_bound(h, w, c), (unsigned long long)sn_png_workspace_size(h, w, c));
        return 0;
    }
    if (cmd == "lengths" && argc > 2) {
        const int n = argc - 2;
        std::vector<uint32_t> counts(n), key(2 * n);
        std::vector<uint16_t> parent(2 * n), codes(n);
        std::vector<uint8_t> lens(n);
        for (int i = 0; i < n; ++i) counts[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 10);
        sn_png_build_lengths(counts.data(), n, lens.data(), key.data(), parent.data());
        uint32_t deepest = 0, kraft = 0, work[32];
        for (int i = 0; i < n; ++i) {
            printf("%u ", lens[i]);
            if (lens[i] > deepest) deepest = lens[i];
            if (lens[i] && lens[i] <= 15) kraft += 1u << (15 - lens[i]);
        }
        printf("\n%u %u\n", deepest, kraft);
        // the canonical codes of a complete code are prefix-free: checked as distinct (reversed code, length) pairs
        if (deepest <= 15) {
            sn_png_canonical_codes(lens.data(), n, codes.data(), work);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < i; ++j)
                    if (lens[i] && lens[j]) {
                        const uint32_t l = lens[i] < lens[j] ? lens[i] : lens[j];
                        if (((codes[i] ^ codes[j]) & ((1u << l) - 1)) == 0) { fprintf(stderr, "codes %d and %d share a prefix\n", j, i); return 3; }
                    }
        }
        return 0;
    }
    if (cmd == "sums" && argc == 5) {
        const std::vector<uint8_t> v = read_file(argv[2]);
        const size_t a = (size_t)atol(argv[3]), b = (size_t)atol(argv[4]), cuts[4] = {0, a, b, v.size()};
        uint32_t crc = 0, adler = 1;
        uint64_t acc_a = 0, acc_b = 0;
        for (int k = 0; k < 3; ++k) {
            const uint8_t* s = v.data() + cuts[k];
            const size_t n = cuts[k + 1] - cuts[k];
            crc = sn_png_crc_combine(crc, sn_png_crc32(s, n), n);
            uint32_t sa = 0, sb = 0;
            for (size_t j = 0; j < n; ++j) {
                sa = (sa + s[j]) % SN_PNG_ADLER_MOD;
                sb = (uint32_t)((sb + (uint64_t)((n - j) % SN_PNG_ADLER_MOD) * s[j]) % SN_PNG_ADLER_MOD);
            }
            adler = sn_png_adler_combine(adler, sn_png_adler_of_sums(sa, sb, n), n);
            sn_png_adler_accumulate(sa, sb, v.size() - cuts[k + 1], acc_a, acc_b);
        }
        printf("%u %u %u\n", crc, adler, sn_png_adler_of_sums((uint32_t)acc_a, (uint32_t)acc_b, v.size()));
        return 0;
    }
    fprintf(stderr, "usage: png_encode encode|plan|lengths|sums ...\n");
    return 1;
}
