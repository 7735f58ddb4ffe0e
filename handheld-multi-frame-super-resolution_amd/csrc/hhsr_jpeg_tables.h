// JPEG output, the part that needs no device (include/hhsr.h "JPEG output"): the tables of T.81 annex K, the geometry of a
// file, Huffman table specifications -> code words (annex C), counts -> an optimal specification (K.2 with libjpeg's
// choices) and the header writer.  Plain C++17 without a HIP include, so that a stand-alone program can compile it under
// a sanitiser (tests/jpeg_tables_driver.cpp); hhsr_jpeg.hip wraps it in the C ABI.
#ifndef HHSR_JPEG_TABLES_H
#define HHSR_JPEG_TABLES_H
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define JPEG_HD __host__ __device__
#else
#define JPEG_HD
#endif

namespace jpeg {
#define JPEG_ZIGZAG                                                                                                    \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,                          \
     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,                          \
     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
#define JPEG_K1_LUMA                                                                                                   \
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,       \
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,       \
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99}
#define JPEG_K2_CHROMA                                                                                                 \
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, \
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}
// (one text each for the host's header writer and the kernels: a host array cannot be indexed by a lane)
constexpr uint8_t ZIGZAG[64] = JPEG_ZIGZAG;  // ZIGZAG[k]: row-major index u * 8 + v of the k-th coefficient
constexpr uint8_t K1_LUMA[64] = JPEG_K1_LUMA;
constexpr uint8_t K2_CHROMA[64] = JPEG_K2_CHROMA;

struct HuffSpec {
    uint8_t bits[16];   // BITS: codes of length 1 .. 16
    int n;              // number of symbols
    uint8_t vals[256];  // HUFFVAL
};
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
// file order: DC luma, AC luma, DC chroma, AC chroma
constexpr const HuffSpec* STANDARD_SPECS[4] = {&DC_LUMA, &AC_LUMA, &DC_CHROMA, &AC_CHROMA};

// The code tables the entropy coder reads, made from four specifications (annex C): entry = code | length << 16, a symbol
// the table does not have = 0.  [0] luma, [1] chroma; DC symbols are the 12 categories, AC symbols run << 4 | size.
struct HuffCodes {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr void huff_fill(const HuffSpec& s, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) out[s.vals[k++]] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
}
// specs: DC luma, AC luma, DC chroma, AC chroma (the chroma pair may be null: one component)
constexpr HuffCodes huff_codes(const HuffSpec* const* specs) {
    HuffCodes h = {};
    huff_fill(*specs[0], h.dc[0]);
    huff_fill(*specs[1], h.ac[0]);
    if (specs[2] != nullptr) huff_fill(*specs[2], h.dc[1]);
    if (specs[3] != nullptr) huff_fill(*specs[3], h.ac[1]);
    return h;
}
constexpr int HUFF_WORDS = sizeof(HuffCodes) / 4;  // 544
constexpr int SPEC_BYTES = 16 + 256;               // a table specification of the C ABI: BITS, then HUFFVAL

// A row of the C ABI's specification -> HuffSpec; false unless it is a table a baseline file may carry: 1 .. 256 symbols,
// none twice, DC symbols <= 11 (they index 16 entries), the code lengths a prefix code (annex C never runs out of codes)
// in which no code is all 1-bits.
inline bool spec_parse(const uint8_t* row, bool dc, HuffSpec* out) {
    int n = 0;
    uint32_t code = 0;
    for (int len = 1; len <= 16; ++len) {
        const int b = row[len - 1];
        out->bits[len - 1] = (uint8_t)b;
        n += b;
        if (code + (uint32_t)b > (1u << len) - (b ? 1u : 0u)) return false;
        code = (code + (uint32_t)b) << 1;
    }
    if (n < 1 || n > 256) return false;
    bool seen[256] = {};
    for (int i = 0; i < 256; ++i) out->vals[i] = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t v = row[16 + i];
        if (seen[v] || (dc && v > 11)) return false;
        seen[v] = true;
        out->vals[i] = v;
    }
    out->n = n;
    return true;
}

// counts[256] -> spec[SPEC_BYTES] by T.81 K.2 as libjpeg runs it (jpeg_gen_optimal_table): a reserved symbol 256 of count
// 1, so that no code is all 1-bits; the two least non-zero counts are merged, ties going to the larger symbol index;
// lengths above 16 shortened by Figure K.3; the reserved symbol removed from the longest length in use; HUFFVAL ordered by
// length, then by symbol.  false: every count is zero, or their sum does not fit 64 bits.
inline bool huffman_build(const uint64_t* counts, uint8_t* spec) {
    uint64_t freq[257], total = 1;
    int codesize[257], others[257];
    for (int i = 0; i < 256; ++i) {
        freq[i] = counts[i];
        if (counts[i] > UINT64_MAX - total) return false;
        total += counts[i];
    }
    if (total == 1) return false;
    freq[256] = 1;
    for (int i = 0; i < 257; ++i) codesize[i] = 0, others[i] = -1;
    for (;;) {
        int c1 = -1, c2 = -1;
        uint64_t v = UINT64_MAX;
        for (int i = 0; i <= 256; ++i)
            if (freq[i] && freq[i] <= v) v = freq[i], c1 = i;
        v = UINT64_MAX;
        for (int i = 0; i <= 256; ++i)
            if (freq[i] && freq[i] <= v && i != c1) v = freq[i], c2 = i;
        if (c2 < 0) break;
        freq[c1] += freq[c2];
        freq[c2] = 0;
        for (++codesize[c1]; others[c1] >= 0; ++codesize[c1]) c1 = others[c1];
        others[c1] = c2;
        for (++codesize[c2]; others[c2] >= 0; ++codesize[c2]) c2 = others[c2];
    }
    int bits[258] = {};  // (a code of 257 symbols is at most 256 bits long)
    for (int i = 0; i <= 256; ++i)
        if (codesize[i]) ++bits[codesize[i]];
    int i = 257;
    for (; i > 16; --i) {  // Figure K.3
        while (bits[i] > 0) {
            int j = i - 2;
            while (bits[j] == 0) --j;
            bits[i] -= 2;
            ++bits[i - 1];
            bits[j + 1] += 2;
            --bits[j];
        }
    }
    while (bits[i] == 0) --i;
    --bits[i];  // the reserved symbol
    for (int k = 0; k < SPEC_BYTES; ++k) spec[k] = 0;
    for (int len = 1; len <= 16; ++len) spec[len - 1] = (uint8_t)bits[len];
    int k = 16;
    for (int len = 1; len <= 256; ++len)
        for (int s = 0; s < 256; ++s)
            if (codesize[s] == len) spec[k++] = (uint8_t)s;
    return true;
}

// IJG quality scaling: the percentage s, then a table entry
inline int q_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }
JPEG_HD inline int q_entry(int base, int scale) {
    const int q = (base * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// ---- geometry shared by the entry points ---------------------------------------------------------------------------------
constexpr int MAX_DIM = 65535;
constexpr int SCAN_GROUP = 2048;          // intervals per workgroup of the offset scan
constexpr size_t BLOCK_MAX_BYTES = 216;   // 64 coefficients x (16-bit code + 11 magnitude bits) / 8
constexpr int HIST_THREADS = 256;         // k_jpeg_histogram: a thread per block, ...
constexpr int HIST_MAX_GROUPS = 512;      // ... at most this many persistent workgroups, one partial table each
constexpr size_t HIST_TABLE_BYTES = 4 * 256 * sizeof(uint64_t);
struct Geom {
    int mcux, mcuy;
    int bpm;  // blocks per MCU: the components (4:4:4) or 6 (4:2:0)
    size_t n_mcu, n_int, n_groups, n_blocks, hist_groups;
    size_t coef_bytes, scratch_bytes, hist_bytes, max_scan;
};
// subsampling 0: 4:4:4, an MCU is 8 x 8 pixels; 1: 4:2:0, 16 x 16 pixels (comps 3)
inline Geom geom(int H, int W, int comps, int restart_mcus, int subsampling = 0) {
    Geom g;
    const int side = subsampling ? 16 : 8;
    g.mcux = (W + side - 1) / side;
    g.mcuy = (H + side - 1) / side;
    g.bpm = subsampling ? 6 : comps;
    g.n_mcu = (size_t)g.mcux * g.mcuy;  // <= 8192^2
    g.n_int = (g.n_mcu + restart_mcus - 1) / restart_mcus;
    g.n_groups = (g.n_int + SCAN_GROUP - 1) / SCAN_GROUP;
    g.n_blocks = g.n_mcu * g.bpm;
    g.coef_bytes = g.n_blocks * 64 * sizeof(int16_t);
    // scratch of the entropy coder: uint64 offsets[n_int] | uint64 group totals[n_groups] | uint32 sizes[n_int]
    g.scratch_bytes = (g.n_int + g.n_groups) * sizeof(uint64_t) + g.n_int * sizeof(uint32_t);
    // ... of the histogram: uint64 partial tables [hist_groups][4][256]
    g.hist_groups = (g.n_blocks + HIST_THREADS - 1) / HIST_THREADS;
    if (g.hist_groups > (size_t)HIST_MAX_GROUPS) g.hist_groups = HIST_MAX_GROUPS;
    g.hist_bytes = g.hist_groups * HIST_TABLE_BYTES;
    g.max_scan = 2 * BLOCK_MAX_BYTES * g.n_blocks + 2 * (g.n_int - 1);
    return g;
}

// ---- header ------------------------------------------------------------------------------------------------------------------
// SOI .. SOS into out.  *length = the header's bytes, always.  0: written; 1: out_capacity is too small (nothing written);
// 2: the bytes written are not the bytes counted.  Arguments are the caller's to check.
inline int write_header(int H, int W, int nc, int quality, int restart_mcus, int subsampling, const HuffSpec* const* specs,
                        uint8_t* out, size_t out_capacity, size_t* length) {
    const Geom g = geom(H, W, nc, restart_mcus, subsampling);
    const bool dri = (size_t)restart_mcus < g.n_mcu;
    const int ntab = nc == 1 ? 1 : 2;
    size_t need = 2 + 18 + (size_t)ntab * 69 + (10 + 3 * nc) + (dri ? 6 : 0) + (8 + 2 * nc);
    for (int t = 0; t < 2 * ntab; ++t) need += 21 + specs[t]->n;
    *length = need;
    if (out_capacity < need) return 1;
    uint8_t* p = out;
    auto u8 = [&](int v) { *p++ = (uint8_t)v; };
    auto u16 = [&](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
    u16(0xFFD8);
    u16(0xFFE0); u16(16);  // APP0: JFIF 1.02, no units, aspect 1:1, no thumbnail
    for (const char c : {'J', 'F', 'I', 'F', '\0'}) u8(c);
    u8(1); u8(2); u8(0); u16(1); u16(1); u8(0); u8(0);
    const int scale = q_scale(quality);
    for (int t = 0; t < ntab; ++t) {
        u16(0xFFDB); u16(67); u8(t);
        for (int k = 0; k < 64; ++k) u8(q_entry((t ? K2_CHROMA : K1_LUMA)[ZIGZAG[k]], scale));
    }
    u16(0xFFC0); u16(8 + 3 * nc); u8(8); u16(H); u16(W); u8(nc);
    for (int c = 0; c < nc; ++c) { u8(c + 1); u8(c == 0 && subsampling ? 0x22 : 0x11); u8(c ? 1 : 0); }
    for (int t = 0; t < 2 * ntab; ++t) {
        const HuffSpec& s = *specs[t];
        u16(0xFFC4); u16(19 + s.n); u8(((t & 1) << 4) | (t >> 1));
        for (int i = 0; i < 16; ++i) u8(s.bits[i]);
        for (int i = 0; i < s.n; ++i) u8(s.vals[i]);
    }
    if (dri) { u16(0xFFDD); u16(4); u16(restart_mcus); }
    u16(0xFFDA); u16(6 + 2 * nc); u8(nc);
    for (int c = 0; c < nc; ++c) { u8(c + 1); u8(c ? 0x11 : 0x00); }
    u8(0); u8(63); u8(0);
    return (size_t)(p - out) == need ? 0 : 2;
}

// spec (C ABI, n_tables rows) or null -> the four table pointers (the chroma pair null with two rows); `store` holds parsed
// rows.  false: a row is no valid table.
inline bool specs_from_abi(const uint8_t* spec, int n_tables, HuffSpec* store, const HuffSpec** specs) {
    for (int t = 0; t < 4; ++t) specs[t] = t < n_tables ? STANDARD_SPECS[t] : nullptr;
    if (spec == nullptr) return true;
    for (int t = 0; t < n_tables; ++t) {
        if (!spec_parse(spec + (size_t)t * SPEC_BYTES, (t & 1) == 0, &store[t])) return false;
        specs[t] = &store[t];
    }
    return true;
}
}  // namespace jpeg
#endif  // HHSR_JPEG_TABLES_H
