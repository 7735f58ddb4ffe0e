// Lossless JPEG (ITU-T T.81 Annex H, SOF3) as DNG Compression 7 wants it written: the per-sample rule (prediction, category,
// code word, magnitude bits), the Huffman table construction of Annex K.2, the fixed part of a tile's stream and the encoder
// of the whole image as a plain host loop.  Like hhsr_ljpeg_core.h it compiles without HIP (tests/ljpeg_enc_main.cpp builds
// it with clang++ under sanitizers); hhsr_ljpeg_enc.hip includes it for the host entry points and the kernels.
// include/hhsr.h, section "DNG output: lossless JPEG", states the contract; this file is its one implementation.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/hhsr.h"

#if defined(__HIPCC__)
#define HHSR_LJE_HD __host__ __device__ __forceinline__
#else
#define HHSR_LJE_HD inline
#endif

namespace hhsr_lje {

constexpr int N_CAT = 17;                          // SSSS 0 .. 16
constexpr int64_t MAX_TILE_SAMPLES = (int64_t)1 << 28;  // tile_h tile_w Nf: what the decoder accepts as one stream
constexpr int64_t MAX_SAMPLES = (int64_t)1 << 40;       // the padded image: counts stay far below 2^64, a workgroup's below 2^32
constexpr int MAX_EDGE = 1 << 30;                 // H and W: a tile's x0 + x and y0 + y stay inside int
constexpr int MAX_BITS = 31;                       // a 16-bit code and the 15 magnitude bits of SSSS 15
constexpr int MAX_HEADER = 2 + 22 + 4 * 38 + 16;   // SOI, SOF3, four DHTs of 17 values, SOS

// The code words as the kernels take them, by value: e[c][ssss] = length << 16 | code, 0 where the table has no code; then
// the bytes every tile's stream begins with (they depend on the tile size, not on the tile).
struct Codes {
    uint32_t e[HHSR_LJPEG_MAX_COMPONENTS][N_CAT];
    uint32_t header_bytes;
    uint8_t header[MAX_HEADER];
};

constexpr int SCAN_GROUP = 2048;       // tiles per workgroup of the offsets scan (= jpeg::SCAN_GROUP, asserted in the .hip)

struct Geom {
    int tiles_x, tiles_y;
    uint64_t n_tiles, n_groups;
    uint64_t tile_samples;    // tile_h tile_w Nf
    uint64_t tile_max_bytes;  // the bound of one tile's slot (hhsr.h)
    uint64_t max_bytes, scratch_bytes;
};

constexpr int HIST_MAX_GROUPS = 1024;  // workgroups of the histogram: one partial table each
constexpr int HIST_STRIDE = 72;        // uint64 per partial table: [4][17] counts, then the bad-sample flag

// false: dimensions or options outside the contract
inline bool geom(int H, int W, int Nf, int tile_h, int tile_w, Geom* g) {
    if (H < 1 || W < 1 || H > MAX_EDGE || W > MAX_EDGE || Nf < 1 || Nf > HHSR_LJPEG_MAX_COMPONENTS) return false;
    if (tile_h < 16 || tile_h > 65535 || tile_w < 16 || tile_w > 65535 || (tile_h & 15) || (tile_w & 15)) return false;
    g->tile_samples = (uint64_t)tile_h * (uint64_t)tile_w * (uint64_t)Nf;
    if (g->tile_samples > (uint64_t)MAX_TILE_SAMPLES) return false;
    g->tiles_x = (int)(((int64_t)W + tile_w - 1) / tile_w);
    g->tiles_y = (int)(((int64_t)H + tile_h - 1) / tile_h);
    g->n_tiles = (uint64_t)g->tiles_x * (uint64_t)g->tiles_y;
    if (g->n_tiles * g->tile_samples > (uint64_t)MAX_SAMPLES) return false;
    g->n_groups = (g->n_tiles + SCAN_GROUP - 1) / SCAN_GROUP;
    const uint64_t header = 2 + (10 + 3 * (uint64_t)Nf) + (uint64_t)Nf * 38 + (8 + 2 * (uint64_t)Nf);
    g->tile_max_bytes = header + 2 * ((g->tile_samples * MAX_BITS + 7) / 8) + 2 + 1;  // < 2^32 for 2^28 samples
    g->max_bytes = g->n_tiles * g->tile_max_bytes;
    const uint64_t enc = g->n_tiles * sizeof(uint32_t) + 8 + g->n_groups * sizeof(uint64_t);
    const uint64_t hist = (uint64_t)HIST_MAX_GROUPS * HIST_STRIDE * sizeof(uint64_t);
    g->scratch_bytes = (enc > hist ? enc : hist) + 8;
    return true;
}

// ---- the per-sample rule (host and device) ------------------------------------------------------------------------------------
// The prediction of the sample at line y, column x of a tile from Ra (left), Rb (above), Rc (above left): T.81 H.1.2.1.
HHSR_LJE_HD int32_t predict(int predictor, int P, int y, int x, int32_t Ra, int32_t Rb, int32_t Rc) {
    if (y == 0) return x == 0 ? (1 << (P - 1)) : Ra;
    if (x == 0) return Rb;
    switch (predictor) {
        case 1: return Ra;
        case 2: return Rb;
        case 3: return Rc;
        case 4: return Ra + Rb - Rc;
        case 5: return Ra + ((Rb - Rc) >> 1);
        case 6: return Rb + ((Ra - Rc) >> 1);
        default: return (Ra + Rb) >> 1;
    }
}

// The difference modulo 2^16 as -32767 .. 32768, and its category SSSS (32768: 16).
HHSR_LJE_HD int category(int32_t sample, int32_t prediction, int32_t* diff) {
    int32_t d = (sample - prediction) & 0xFFFF;
    if (d > 32768) d -= 65536;
    *diff = d;
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    return a ? 32 - __builtin_clz(a) : 0;
}

// The bits of one sample: the code word of its category (entry = length << 16 | code), then the SSSS low bits of the
// difference (difference - 1 when negative), none for SSSS 0 and 16.  *len = 0: the table has no code for the category.
HHSR_LJE_HD void sample_bits(int32_t sample, int32_t prediction, const uint32_t* entries, uint32_t* val, uint32_t* len) {
    int32_t d;
    const int ssss = category(sample, prediction, &d);
    const uint32_t e = entries[ssss];
    const int nx = ssss == 16 ? 0 : ssss;
    const uint32_t extra = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << nx) - 1u);
    *val = ((e & 0xFFFFu) << nx) | extra;
    *len = (e >> 16) ? (e >> 16) + (uint32_t)nx : 0u;
}

// s(y, x, c) of tile (y0, x0): the image's sample with the edge replicated
HHSR_LJE_HD int32_t tile_sample(const uint16_t* img, int H, int W, int Nf, int64_t row_elems, int y0, int x0, int y, int x, int c) {
    const int iy = y0 + y < H ? y0 + y : H - 1, ix = x0 + x < W ? x0 + x : W - 1;
    return img[(int64_t)iy * row_elems + (int64_t)ix * Nf + c];
}

// ---- Annex K.2 (host) -----------------------------------------------------------------------------------------------------------
// 17 counts -> bits[16], values[17] (unused ones 0), *n_values: figures K.1 to K.4 with the reserved code point.  false when
// no count is set or their sum passes 2^62.
inline bool build_k2(const uint64_t* counts, uint8_t* bits_out, uint8_t* values_out, int* n_values) {
    constexpr int N = N_CAT + 1;
    uint64_t f[N], sum = 0;
    for (int i = 0; i < N_CAT; ++i) {
        f[i] = counts[i];
        if (counts[i] > ((uint64_t)1 << 62) || (sum += counts[i]) > ((uint64_t)1 << 62)) return false;
    }
    if (sum == 0) return false;
    f[N_CAT] = 1;  // the reserved code point
    int codesize[N], others[N];
    for (int i = 0; i < N; ++i) codesize[i] = 0, others[i] = -1;
    for (;;) {  // figure K.1: the least two frequencies, of equal ones the larger index
        int v1 = -1, v2 = -1;
        for (int i = 0; i < N; ++i)
            if (f[i] > 0 && (v1 < 0 || f[i] <= f[v1])) v1 = i;
        for (int i = 0; i < N; ++i)
            if (f[i] > 0 && i != v1 && (v2 < 0 || f[i] <= f[v2])) v2 = i;
        if (v2 < 0) break;
        f[v1] += f[v2];
        f[v2] = 0;
        ++codesize[v1];
        while (others[v1] >= 0) {
            v1 = others[v1];
            ++codesize[v1];
        }
        others[v1] = v2;
        ++codesize[v2];
        while (others[v2] >= 0) {
            v2 = others[v2];
            ++codesize[v2];
        }
    }
    int bits[33];
    for (int i = 0; i < 33; ++i) bits[i] = 0;
    for (int i = 0; i < N; ++i)
        if (codesize[i]) {
            if (codesize[i] > 32) return false;  // (18 symbols: at most 17)
            ++bits[codesize[i]];
        }
    int i = 32;  // figure K.3
    for (; i > 16; --i) {
        while (bits[i] > 0) {
            int j = i - 2;
            while (bits[j] == 0) --j;
            bits[i] -= 2;
            bits[i - 1] += 1;
            bits[j + 1] += 2;
            bits[j] -= 1;
        }
    }
    while (bits[i] == 0) --i;
    --bits[i];  // the reserved code point leaves
    for (int l = 1; l <= 16; ++l) bits_out[l - 1] = (uint8_t)bits[l];
    int k = 0;  // figure K.4
    for (int size = 1; size <= 32; ++size)
        for (int v = 0; v < N_CAT; ++v)
            if (codesize[v] == size) values_out[k++] = (uint8_t)v;
    *n_values = k;
    for (; k < N_CAT; ++k) values_out[k] = 0;
    return true;
}

// ---- code words and the fixed bytes of a tile's stream (host) ----------------------------------------------------------------------
// bits [Nf][16], values [Nf][17] -> codes (Annex C) and the header.  false: lengths that are no prefix code, no value or more
// than 17, a value above 16 or named twice.
inline bool make_codes(const uint8_t* bits, const uint8_t* values, int Nf, int P, int predictor, int tile_h, int tile_w, Codes* out) {
    *out = Codes{};
    uint8_t* h = out->header;
    uint32_t n = 0;
    auto put = [&](int b) { h[n++] = (uint8_t)b; };
    auto put16 = [&](int v) { put(v >> 8), put(v & 255); };
    put(0xFF), put(0xD8);
    put(0xFF), put(0xC3), put16(8 + 3 * Nf), put(P), put16(tile_h), put16(tile_w), put(Nf);
    for (int c = 0; c < Nf; ++c) put(c + 1), put(0x11), put(0);
    for (int c = 0; c < Nf; ++c) {
        const uint8_t* b = bits + 16 * c;
        const uint8_t* v = values + 17 * c;
        int total = 0;
        uint32_t kraft = 0, seen = 0;
        for (int l = 1; l <= 16; ++l) {
            total += b[l - 1];
            kraft += (uint32_t)b[l - 1] << (16 - l);
        }
        if (total < 1 || total > N_CAT || kraft > 65536u) return false;
        uint32_t code = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < b[l - 1]; ++i, ++k, ++code) {
                if (v[k] > 16 || (seen >> v[k] & 1u)) return false;
                seen |= 1u << v[k];
                out->e[c][v[k]] = (uint32_t)l << 16 | code;
            }
            code <<= 1;
        }
        put(0xFF), put(0xC4), put16(2 + 1 + 16 + total), put(c);
        for (int l = 0; l < 16; ++l) put(b[l]);
        for (int i = 0; i < total; ++i) put(v[i]);
    }
    put(0xFF), put(0xDA), put16(6 + 2 * Nf), put(Nf);
    for (int c = 0; c < Nf; ++c) put(c + 1), put(c << 4);
    put(predictor), put(0), put(0);
    out->header_bytes = n;
    return true;
}

// ---- the whole image on the host: hhsr_ljpeg_encode_host ---------------------------------------------------------------------------
struct ByteSink {  // out[0 .. capacity): what lies behind is counted and not stored
    uint8_t* out;
    uint64_t capacity, at;
    void put(uint32_t b) {
        if (at < capacity) out[at] = (uint8_t)b;
        ++at;
    }
};

inline void encode_image(const uint16_t* img, int H, int W, int Nf, int64_t row_elems, int P, int predictor, int tile_h,
                         int tile_w, const Codes& codes, const Geom& g, uint8_t* out, uint64_t capacity, uint64_t* offsets,
                         uint32_t* tile_bytes, uint64_t* length) {
    ByteSink sink{out, capacity, 0};
    bool bad = false;  // a category without a code, a sample at or above 2^P
    for (int ty = 0; ty < g.tiles_y; ++ty) {
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            const uint64_t t = (uint64_t)ty * g.tiles_x + tx, start = sink.at;
            const int y0 = ty * tile_h, x0 = tx * tile_w;
            offsets[t] = start;
            for (uint32_t i = 0; i < codes.header_bytes; ++i) sink.put(codes.header[i]);
            uint64_t acc = 0;  // the low nacc bits wait for a whole byte
            int nacc = 0;
            for (int y = 0; y < tile_h; ++y) {
                for (int x = 0; x < tile_w; ++x) {
                    for (int c = 0; c < Nf; ++c) {
                        const int32_t s = tile_sample(img, H, W, Nf, row_elems, y0, x0, y, x, c);
                        const int32_t Ra = x ? tile_sample(img, H, W, Nf, row_elems, y0, x0, y, x - 1, c) : 0;
                        const int32_t Rb = y ? tile_sample(img, H, W, Nf, row_elems, y0, x0, y - 1, x, c) : 0;
                        const int32_t Rc = x && y ? tile_sample(img, H, W, Nf, row_elems, y0, x0, y - 1, x - 1, c) : 0;
                        uint32_t val, len;
                        sample_bits(s, predict(predictor, P, y, x, Ra, Rb, Rc), codes.e[c], &val, &len);
                        bad |= len == 0 || (s >> P) != 0;
                        acc = (acc << len) | val;
                        nacc += (int)len;
                        while (nacc >= 8) {
                            const uint32_t b = (uint32_t)(acc >> (nacc - 8)) & 255u;
                            sink.put(b);
                            if (b == 255u) sink.put(0);
                            nacc -= 8;
                        }
                    }
                }
            }
            if (nacc > 0) {  // padded with 1-bits
                const uint32_t b = (uint32_t)((acc << (8 - nacc)) | (255u >> nacc)) & 255u;
                sink.put(b);
                if (b == 255u) sink.put(0);
            }
            sink.put(0xFF), sink.put(0xD9);
            tile_bytes[t] = (uint32_t)(sink.at - start);
            if ((sink.at - start) & 1) sink.put(0);  // the next stream starts at an even offset
        }
    }
    offsets[g.n_tiles] = sink.at;
    *length = bad ? UINT64_MAX : sink.at;
}

}  // namespace hhsr_lje
